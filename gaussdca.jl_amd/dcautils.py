"""Host-side mirror of the DCAUtils.jl operator surface that GaussDCA.jl calls
(/root/reference/src/GaussDCA.jl:20,22,28,30,37,39) plus the in-tree helpers compute_C (:76),
correct_APC (:78-86) and compute_ranking (:88-99).  Same names, argument meaning, return
shapes and error behaviour; the arithmetic of every hot operator runs in libgdca.so on the
MI355X (no CPU fallback).  FASTA parsing, deduplication and the ranking sort are host code,
as they are in the reference.

Array conventions follow Julia: ``Z`` has shape ``(N, M)`` (column = sequence) and is passed
Fortran-contiguous, i.e. the same bytes as Julia's ``Matrix{Int8}``; indices in rankings are
1-based.
"""
from __future__ import annotations

import ctypes as C
import gzip
import math
from collections.abc import Sequence as _SequenceABC
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import ArgumentError, PosDefException, default_context  # noqa: F401

_LETTERS = "ACDEFGHIKLMNPQRSTVWY"
_L2N = np.full(256, 21, dtype=np.int8)
for _i, _c in enumerate(_LETTERS):
    _L2N[ord(_c)] = _i + 1


def _zf(Z) -> np.ndarray:
    Z = np.asarray(Z)
    if Z.ndim != 2:
        raise ArgumentError("Z must be an N x M matrix")
    return np.asfortranarray(Z, dtype=np.int8)


def _theta_arg(theta) -> float:
    """theta = :auto | Real in [0, 1]  ->  the C-ABI's encoding (negative = auto)."""
    if isinstance(theta, str):
        if theta.lstrip(":") == "auto":
            return -1.0
        raise ArgumentError(f"invalid θ value: {theta} (must be either :auto, or a number between 0 and 1)")
    if isinstance(theta, (int, float, np.integer, np.floating)) and 0 <= theta <= 1:
        return float(theta)
    raise ArgumentError(f"invalid θ value: {theta} (must be either :auto, or a number between 0 and 1)")


# ---- host I/O (reference: DCAUtils.read_fasta_alignment, src/GaussDCA.jl:20) -----------------------
# ---- native host utilities (libgdca.so, plain C++; pure-Python statements of the same rules: tests/host_mirrors.py) ----
def read_fasta_alignment(filename: str, max_gap_fraction: float) -> np.ndarray:
    """read_fasta_alignment(filename, max_gap_fraction) -> Z::Matrix{Int8}, shape (N, M), Fortran order
    (reference call site src/GaussDCA.jl:20)."""
    lib = _lib.load()
    h = C.c_void_p()
    N, M = C.c_int32(), C.c_int32()
    st = lib.gdca_fasta_open(str(filename).encode(), float(max_gap_fraction), C.byref(h), C.byref(N), C.byref(M))
    if st != 0:
        raise ValueError(f"cannot read FASTA alignment {filename} (empty, unreadable or not aligned)")
    try:
        Z = np.empty((N.value, M.value), dtype=np.int8, order="F")
        lib.gdca_fasta_copy(h, _lib._p(Z))
    finally:
        lib.gdca_fasta_close(h)
    return Z


class FastaAlignment:
    """A parsed alignment kept where the native reader put it (gdca_fasta_open): `.ptr` = the N x M int8 matrix
    (gdca_fasta_data), `.N`, `.M`, `.q` = maximum(Z) (gdca_fasta_max_symbol).  A context manager: the matrix is freed on exit."""

    def __init__(self, filename: str, max_gap_fraction: float):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        N, M = C.c_int32(), C.c_int32()
        st = self.lib.gdca_fasta_open(str(filename).encode(), float(max_gap_fraction), C.byref(self.h), C.byref(N), C.byref(M))
        if st != 0:
            self.h = None
            raise ValueError(f"cannot read FASTA alignment {filename} (empty, unreadable or not aligned)")
        self.N, self.M = int(N.value), int(M.value)
        self.ptr = int(self.lib.gdca_fasta_data(self.h) or 0)
        self.q = int(self.lib.gdca_fasta_max_symbol(self.h))

    def close(self):
        if self.h:
            self.lib.gdca_fasta_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def remove_duplicate_sequences(Z) -> Tuple[np.ndarray, np.ndarray]:
    """-> (Z without repeated columns, 1-based indices kept)  (reference call site src/GaussDCA.jl:21-23)"""
    lib = _lib.load()
    Zf = _zf(Z)
    N, M = Zf.shape
    out = np.empty((N, M), dtype=np.int8, order="F")
    idx = np.empty(M, dtype=np.int32)
    m = C.c_int32()
    st = lib.gdca_remove_duplicates(_lib._p(Zf), N, M, _lib._p(out), _lib._p(idx), C.byref(m))
    if st != 0:
        raise ArgumentError("remove_duplicate_sequences: invalid arguments")
    return np.asfortranarray(out[:, :m.value]), idx[:m.value].astype(np.int64)


class Ranking(_SequenceABC):
    """The ranking as a sequence of (i, j, score) tuples (what the reference returns as a
    Vector{Tuple{Int,Int,Float64}}), backed by the three arrays the native sort filled: building
    122 760 Python tuples costs more than the sort, so they are made on access.  `.i`, `.j`, `.score`
    are the arrays; slicing gives a list of tuples; comparing with a list compares element-wise."""

    __slots__ = ("i", "j", "score")

    def __init__(self, i, j, score):
        self.i, self.j, self.score = i, j, score

    def __len__(self):
        return int(self.i.shape[0])

    def __getitem__(self, t):
        if isinstance(t, slice):
            return list(zip(self.i[t].tolist(), self.j[t].tolist(), self.score[t].tolist()))
        return (int(self.i[t]), int(self.j[t]), float(self.score[t]))

    def __iter__(self):
        return iter(zip(self.i.tolist(), self.j.tolist(), self.score.tolist()))

    def __eq__(self, other):
        try:
            return len(self) == len(other) and all(a == tuple(b) for a, b in zip(self, other))
        except TypeError:
            return NotImplemented

    def __repr__(self):
        head = ", ".join(repr(x) for x in self[:3])
        return f"Ranking(len={len(self)}: [{head}{', ...' if len(self) > 3 else ''}])"


def compute_ranking(S, min_separation: int = 5) -> "Ranking":
    """compute_ranking(S, min_separation)  (src/GaussDCA.jl:88-99): 1-based (i, j, S[j, i]), stable sort by
    `isless` on the score, reversed (NaN first, 0.0 before -0.0, exact ties in generation order)."""
    lib = _lib.load()
    Sf = np.asfortranarray(S, dtype=np.float64)
    N = Sf.shape[0]
    n = int(lib.gdca_ranking_length(N, int(min_separation)))
    if n <= 0:
        return Ranking(np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.float64))
    ii = np.empty(n, dtype=np.int32)
    jj = np.empty(n, dtype=np.int32)
    sc = np.empty(n, dtype=np.float64)
    st = lib.gdca_ranking(_lib._p(Sf), N, int(min_separation), _lib._p(ii), _lib._p(jj), _lib._p(sc))
    if st != 0:
        raise ArgumentError("compute_ranking: invalid arguments")
    return Ranking(ii, jj, sc)


# ---- hot operators (libgdca.so) -----------------------------------------------------------------------
def compute_theta(Z, ctx=None) -> float:
    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    th = C.c_double()
    ctx.check(ctx.lib.gdca_compute_theta(ctx.h, _lib._p(Zf), N, M, C.byref(th)))
    return th.value


def pair_identity_sum(Z, ctx=None) -> int:
    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    out = C.c_uint64()
    ctx.check(ctx.lib.gdca_pair_identity_sum(ctx.h, _lib._p(Zf), N, M, C.byref(out)))
    return int(out.value)


def neighbour_counts(Z, thresh: int, ctx=None) -> np.ndarray:
    """n_k = 1 + #{l != k : Hamming(Z[:,k], Z[:,l]) < thresh}, int32[M] (bit-exact integers)."""
    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    n = np.empty(M, dtype=np.int32)
    ctx.check(ctx.lib.gdca_neighbour_counts(ctx.h, _lib._p(Zf), N, M, int(thresh), _lib._p(n)))
    return n


def compute_weights(Z, q=None, theta=":auto", ctx=None, return_theta: bool = False):
    """compute_weights(Z, [q,] θ) -> (W, Meff).  ``q`` is accepted for signature compatibility
    (DCAUtils uses it to pick its bit-packed path) and checked against the q <= 31 limit."""
    if q is not None and not isinstance(q, (int, np.integer)):
        q, theta = None, q  # called as compute_weights(Z, θ)
    if q is not None and q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    W = np.empty(M, dtype=np.float64)
    Meff, th, thr = C.c_double(), C.c_double(), C.c_int32()
    ctx.check(ctx.lib.gdca_compute_weights(ctx.h, _lib._p(Zf), N, M, _theta_arg(theta), _lib._p(W), C.byref(Meff),
                                           C.byref(th), C.byref(thr)))
    if return_theta:
        return W, Meff.value, th.value, int(thr.value)
    return W, Meff.value


def compute_weighted_frequencies(Z, q_or_W, theta_or_Meff=":auto", ctx=None):
    """compute_weighted_frequencies(Z, q, θ) -> (Pi_true, Pij_true, Meff, W)   (src/GaussDCA.jl:28)
    compute_weighted_frequencies(Z, W, Meff) -> (Pi_true, Pij_true)           (DCAUtils' 2nd method)"""
    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    if isinstance(q_or_W, (int, np.integer)):
        q = int(q_or_W)
        if q >= 32:
            raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
        W, Meff = compute_weights(Zf, q, theta_or_Meff, ctx=ctx)
        Pi, Pij = _frequencies(ctx, Zf, q, W, Meff)
        return Pi, Pij, Meff, W
    W = np.ascontiguousarray(q_or_W, dtype=np.float64)
    q = int(Zf.max())
    return _frequencies(ctx, Zf, q, W, float(theta_or_Meff))


def _frequencies(ctx, Zf, q, W, Meff):
    N, M = Zf.shape
    n = N * (q - 1)
    Pi = np.empty(n, dtype=np.float64)
    Pij = np.empty((n, n), dtype=np.float64)
    ctx.check(ctx.lib.gdca_frequencies(ctx.h, _lib._p(Zf), N, M, q, _lib._p(W), float(Meff), _lib._p(Pi),
                                       _lib._p(Pij)))
    return Pi, Pij


def add_pseudocount(Pi_true, Pij_true, pc: float, q: int = 21, ctx=None):
    """add_pseudocount(Pi_true, Pij_true, pc, q) -> (Pi, Pij)   (src/GaussDCA.jl:30)"""
    ctx = ctx or default_context()
    Pi_true = np.ascontiguousarray(Pi_true, dtype=np.float64)
    Pij_true = np.ascontiguousarray(Pij_true, dtype=np.float64)
    n = Pi_true.shape[0]
    if Pij_true.shape != (n, n) or n % (q - 1) != 0:
        raise ArgumentError("incompatible sizes of Pi, Pij and q")
    N = n // (q - 1)
    Pi = np.empty_like(Pi_true)
    Pij = np.empty_like(Pij_true)
    ctx.check(ctx.lib.gdca_add_pseudocount(ctx.h, _lib._p(Pi_true), _lib._p(Pij_true), N, int(q), float(pc),
                                           _lib._p(Pi), _lib._p(Pij)))
    return Pi, Pij


def compute_C(Pi, Pij, ctx=None) -> np.ndarray:
    """compute_C(Pi, Pij) = Pij - Pi * Pi'   (src/GaussDCA.jl:76)"""
    ctx = ctx or default_context()
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    Pij = np.ascontiguousarray(Pij, dtype=np.float64)
    n = Pi.shape[0]
    Cm = np.empty((n, n), dtype=np.float64)
    ctx.check(ctx.lib.gdca_covariance(ctx.h, _lib._p(Pi), _lib._p(Pij), n, _lib._p(Cm)))
    return Cm


def inv_cholesky(Cm, ctx=None, return_logdet: bool = False):
    """mJ = inv(cholesky(C))   (src/GaussDCA.jl:34).  Raises PosDefException(info) like Julia.
    return_logdet=True: (mJ, log det C) -- the sum of the logarithms of the pivots the inverse met on its way (2 sum log diag of the
    Cholesky factor), the constant sequence_loglik needs; mJ is the same bits either way."""
    ctx = ctx or default_context()
    A = np.array(Cm, dtype=np.float64, order="C", copy=True)
    n = A.shape[0]
    if A.shape != (n, n) or not np.array_equal(A, A.T):
        raise PosDefException(-1)
    info = C.c_int32()
    if return_logdet:
        logdet = C.c_double(float("nan"))
        rc = ctx.lib.gdca_spd_inverse_logdet(ctx.h, _lib._p(A), n, C.byref(info), C.byref(logdet))
        ctx.check(rc, info.value)
        return A, logdet.value
    rc = ctx.lib.gdca_spd_inverse(ctx.h, _lib._p(A), n, C.byref(info))
    ctx.check(rc, info.value)
    return A


def compute_FN(mJ, q: int = 21, ctx=None) -> np.ndarray:
    """compute_FN(mJ, q) -> N x N   (src/GaussDCA.jl:39)"""
    ctx = ctx or default_context()
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    N = mJ.shape[0] // (q - 1)
    S = np.empty((N, N), dtype=np.float64)
    ctx.check(ctx.lib.gdca_fn(ctx.h, _lib._p(mJ), N, int(q), _lib._p(S)))
    return S


def compute_DI_gauss(mJ, Cm, q: int = 21, ctx=None) -> np.ndarray:
    """compute_DI_gauss(mJ, C, q) -> N x N   (src/GaussDCA.jl:37)"""
    ctx = ctx or default_context()
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    N = mJ.shape[0] // (q - 1)
    S = np.empty((N, N), dtype=np.float64)
    ctx.check(ctx.lib.gdca_di(ctx.h, _lib._p(mJ), _lib._p(Cm), N, int(q), _lib._p(S)))
    return S


def correct_APC(S, ctx=None) -> np.ndarray:
    """correct_APC(S)   (src/GaussDCA.jl:78-86)"""
    ctx = ctx or default_context()
    A = np.array(S, dtype=np.float64, order="C", copy=True)
    ctx.check(ctx.lib.gdca_apc(ctx.h, _lib._p(A), A.shape[0]))
    return A


def sequence_energies(mJ, Pi, X, q: int = 21, ctx=None) -> np.ndarray:
    """E[k] = 1/2 (x_k - Pi)' mJ (x_k - Pi) for the K columns of X (shape (N, K) like Z, symbols 1..q, q = the gap): minus the
    log-likelihood of each sequence under the Gaussian model with precision mJ = inv(cholesky(C)) (src/GaussDCA.jl:34) and mean
    Pi (add_pseudocount's Pi, :30), up to the model's constant 1/2 log det(2 pi C) (sequence_loglik adds it).  Lower = fits better.
    mJ must be symmetric (its lower triangle is read)."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    Xa = np.asarray(X)
    if Xa.dtype != np.int8 and Xa.ndim == 2:  # (a wider type is not cast blindly: 261 would wrap to the legal symbol 5)
        if not np.issubdtype(Xa.dtype, np.integer) or (Xa.size and (Xa.min() < 1 or Xa.max() > 31)):
            raise ArgumentError("X must hold integer symbols between 1 and q")
    Xf = _zf(Xa)
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if mJ.shape != (n, n) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites, q = {q}, so mJ must be {n} x {n} and Pi have {n} entries "
                            f"(got {mJ.shape} and {Pi.shape})")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    ctx = ctx or default_context()
    E = np.empty(K, dtype=np.float64)
    ctx.check(ctx.lib.gdca_energies(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xf), K, _lib._p(E)))
    return E


LOG_2PI = 1.8378770664093453  # log(2 pi), GDCA_LOG_2PI of include/gdca.h


def loglik_constant(n: int, logdet: float) -> float:
    """c = 1/2 (n log 2 pi + log det C), rounded operation by operation as the library forms it (gdca_run_loglik)."""
    return float(np.float64(0.5) * (np.float64(n) * np.float64(LOG_2PI) + np.float64(logdet)))


def sequence_loglik(mJ, Pi, X, logdet: float, q: int = 21, ctx=None) -> np.ndarray:
    """log p(x_k) = -E(x_k) - 1/2 (n log 2 pi + log det C) for the K columns of X: the density of the Gaussian model N(Pi, C) at the
    one-hot point, comparable across models.  mJ, Pi, X, q as sequence_energies takes them; logdet = log det C, from
    inv_cholesky(C, return_logdet=True).  Host arithmetic on sequence_energies: L = -(E + c)."""
    E = sequence_energies(mJ, Pi, X, q=q, ctx=ctx)
    return -(E + loglik_constant(np.asarray(Pi).shape[0], logdet))


def _what_arg(what) -> int:
    w = str(what).lstrip(":")
    if w == "energy":
        return _lib.PAIR_ENERGY
    if w == "coupling":
        return _lib.PAIR_COUPLING
    raise ArgumentError(f"invalid what value: {what} (must be either energy or coupling)")


def _symbols(X, name: str, dims: str = "a sites x K") -> np.ndarray:
    """(sites, K) symbols -> int8, column-major; a wider type is not cast blindly (261 would wrap to the legal symbol 5)"""
    Xa = np.asarray(X)
    if Xa.ndim != 2:
        raise ArgumentError(f"{name} must be {dims} matrix")
    if Xa.dtype != np.int8:
        if not np.issubdtype(Xa.dtype, np.integer) or (Xa.size and (Xa.min() < 1 or Xa.max() > 31)):
            raise ArgumentError(f"{name} must hold integer symbols between 1 and q")
    return np.asfortranarray(Xa, dtype=np.int8)


def pair_energies(mJ, Pi, XA, XB, q: int = 21, what="energy", ctx=None) -> np.ndarray:
    """E[a, b] for every pairing of the K_A columns of XA (shape (split, K_A): the sites of protein A) with the K_B columns of XB
    (shape (N - split, K_B): protein B) under the Gaussian model (mJ, Pi) of the concatenated alignment -- what partner matching
    ranks candidate pairings by.  ``what="energy"``: the energy ``sequence_energies`` gives the concatenation a (+) b;
    ``what="coupling"``: only its part that depends on the pairing, R[a, b] = sum of mJ[r(j), r(i)] over the non-gap sites i of a
    and j of b (``Pi`` may then be None), with E(a (+) b) = E(a (+) gaps) + E(gaps (+) b) - c0 / 2 + R(a, b).  Returns a
    (K_A, K_B) array.  mJ must be symmetric (its lower triangle is read)."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    w = _what_arg(what)
    Pi = None if (Pi is None and w == _lib.PAIR_COUPLING) else np.ascontiguousarray(Pi, dtype=np.float64)
    XAf, XBf = _symbols(XA, "XA"), _symbols(XB, "XB")
    split, KA = XAf.shape
    NB, KB = XBf.shape
    N = split + NB
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if split < 1 or NB < 1 or mJ.shape != (n, n) or (Pi is not None and Pi.shape != (n,)):
        raise ArgumentError(f"incompatible sizes: XA has {split} sites and XB {NB}, q = {q}, so mJ must be {n} x {n} and Pi have {n} "
                            f"entries (got {mJ.shape} and {None if Pi is None else Pi.shape})")
    if KA < 1 or KB < 1:
        raise ArgumentError("XA or XB holds no sequence")
    ctx = ctx or default_context()
    E = np.empty((KA, KB), dtype=np.float64, order="F")
    ctx.check(ctx.lib.gdca_pair_energies(ctx.h, _lib._p(mJ), _lib._p(Pi) if Pi is not None else None, N, int(q), split, _lib._p(XAf), KA,
                                         _lib._p(XBf), KB, w, _lib._p(E)))
    return E


def species_blocks(labels_a, labels_b):
    """Sequences grouped by species, as the blocked entry points take them.  ``labels_a`` / ``labels_b``: one integer label per
    sequence of A / of B.  Returns ``(perm_a, perm_b, offA, offB, labels)``: ``labels`` the sorted union of both sides' labels
    (species s = labels[s]); ``perm_a`` the stable order that sorts A's sequences by species (``XA[:, perm_a]`` is species-sorted, and
    inside a species the caller's order is kept), likewise ``perm_b``; ``offA`` / ``offB`` int32 offsets of S + 1 entries: species s
    owns the sorted sequences offA[s] .. offA[s + 1] - 1 (none, where a label occurs on the other side only).  Pure numpy."""
    la, lb = np.asarray(labels_a), np.asarray(labels_b)
    for lab in (la, lb):
        if lab.ndim != 1 or (lab.size and not np.issubdtype(lab.dtype, np.integer)):
            raise ArgumentError("species labels must be a vector of integers, one per sequence")
    la, lb = la.astype(np.int64), lb.astype(np.int64)
    labels = np.union1d(la, lb)
    if labels.size < 1:
        raise ArgumentError("species labels hold no sequence")
    perm_a, perm_b = np.argsort(la, kind="stable"), np.argsort(lb, kind="stable")
    offA = np.concatenate(([0], np.searchsorted(la[perm_a], labels, side="right"))).astype(np.int32)
    offB = np.concatenate(([0], np.searchsorted(lb[perm_b], labels, side="right"))).astype(np.int32)
    return perm_a, perm_b, offA, offB, labels


def _block_views(E, offA, offB):
    """the per-species kA_s x kB_s matrices of a packed blocked array, as views of it"""
    out, at = [], 0
    for ka, kb in zip(np.diff(offA).tolist(), np.diff(offB).tolist()):
        out.append(E[at:at + ka * kb].reshape((ka, kb), order="F"))
        at += ka * kb
    return out


def pair_energies_blocked(mJ, Pi, XA, XB, species_a, species_b, q: int = 21, what="energy", ctx=None) -> list:
    """``pair_energies`` for partner matching per species: only the pairings of sequences of A and of B that carry the same species
    label are computed, in one pass (``species_a`` / ``species_b``: one integer label per column of XA / XB, in any order).  Returns a
    list of matrices, one per species in ascending order of the labels (``species_blocks(species_a, species_b)[4]``): entry s is the
    (kA_s, kB_s) matrix of that species' pairings, rows and columns in the caller's order of its sequences, a view of one packed
    array.  Every entry is bit for bit the entry ``pair_energies`` gives that pairing."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    w = _what_arg(what)
    Pi = None if (Pi is None and w == _lib.PAIR_COUPLING) else np.ascontiguousarray(Pi, dtype=np.float64)
    XAf, XBf = _symbols(XA, "XA"), _symbols(XB, "XB")
    split, KA = XAf.shape
    NB, KB = XBf.shape
    N = split + NB
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if split < 1 or NB < 1 or mJ.shape != (n, n) or (Pi is not None and Pi.shape != (n,)):
        raise ArgumentError(f"incompatible sizes: XA has {split} sites and XB {NB}, q = {q}, so mJ must be {n} x {n} and Pi have {n} "
                            f"entries (got {mJ.shape} and {None if Pi is None else Pi.shape})")
    if KA < 1 or KB < 1:
        raise ArgumentError("XA or XB holds no sequence")
    perm_a, perm_b, offA, offB, _ = species_blocks(species_a, species_b)
    if len(perm_a) != KA or len(perm_b) != KB:
        raise ArgumentError(f"species_a / species_b have {len(perm_a)} / {len(perm_b)} labels, XA / XB hold {KA} / {KB} sequences")
    XAs, XBs = np.asfortranarray(XAf[:, perm_a]), np.asfortranarray(XBf[:, perm_b])
    ctx = ctx or default_context()
    E = np.empty(int(np.sum(np.diff(offA).astype(np.int64) * np.diff(offB))), dtype=np.float64)
    ctx.check(ctx.lib.gdca_pair_energies_blocked(ctx.h, _lib._p(mJ), _lib._p(Pi) if Pi is not None else None, N, int(q), split, _lib._p(XAs),
                                                 KA, _lib._p(XBs), KB, _lib._p(offA), _lib._p(offB), len(offA) - 1, w, _lib._p(E)))
    return _block_views(E, offA, offB)


def logodds_information(logdet: float, logdet_a: float, logdet_b: float) -> float:
    """I = -1/2 (log det C - log det C_AA - log det C_BB), rounded operation by operation as the library forms it (gdca_run_pair_logodds):
    the Gaussian mutual information of the halves, the expected log-odds of a native pair."""
    return float(np.float64(-0.5) * ((np.float64(logdet) - np.float64(logdet_a)) - np.float64(logdet_b)))


def _logodds_args(mJ, mJA, mJB, Pi, XA, XB, q):
    """the operator log-odds' arrays as the library takes them, their sizes held against each other"""
    mJ, mJA, mJB = (np.ascontiguousarray(m, dtype=np.float64) for m in (mJ, mJA, mJB))
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    XAf, XBf = _symbols(XA, "XA"), _symbols(XB, "XB")
    split, KA = XAf.shape
    NB, KB = XBf.shape
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    s = int(q) - 1
    n, nA, nB = (split + NB) * s, split * s, NB * s
    if split < 1 or NB < 1 or mJ.shape != (n, n) or mJA.shape != (nA, nA) or mJB.shape != (nB, nB) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: XA has {split} sites and XB {NB}, q = {q}, so mJ, mJA, mJB must be {n} x {n}, {nA} x {nA}, "
                            f"{nB} x {nB} and Pi have {n} entries (got {mJ.shape}, {mJA.shape}, {mJB.shape} and {Pi.shape})")
    if KA < 1 or KB < 1:
        raise ArgumentError("XA or XB holds no sequence")
    return mJ, mJA, mJB, Pi, XAf, XBf, split + NB, split, KA, KB


def pair_logodds(mJ, mJA, mJB, Pi, XA, XB, information: float, q: int = 21, ctx=None) -> np.ndarray:
    """L[a, b] = log p_AB(a (+) b) - log p_A(a) - log p_B(b) for every pairing of the columns of XA with those of XB (as
    ``pair_energies`` takes them) under the joint model (mJ = inv(C), Pi) and the two marginal models mJA = inv(C_AA), mJB =
    inv(C_BB) -- the true marginals, not the diagonal blocks of mJ; ``information`` = ``logodds_information`` of the three log dets.
    L = ((EmA[a] + EmB[b]) - E[a, b]) + I with the marginal and the joint energies.  Higher = more likely partners.  Returns a
    (K_A, K_B) array.  The matrices must be symmetric (their lower triangles are read)."""
    mJ, mJA, mJB, Pi, XAf, XBf, N, split, KA, KB = _logodds_args(mJ, mJA, mJB, Pi, XA, XB, q)
    ctx = ctx or default_context()
    L = np.empty((KA, KB), dtype=np.float64, order="F")
    ctx.check(ctx.lib.gdca_pair_logodds(ctx.h, _lib._p(mJ), _lib._p(mJA), _lib._p(mJB), _lib._p(Pi), N, int(q), split, _lib._p(XAf), KA,
                                        _lib._p(XBf), KB, float(information), _lib._p(L)))
    return L


def pair_logodds_blocked(mJ, mJA, mJB, Pi, XA, XB, species_a, species_b, information: float, q: int = 21, ctx=None) -> list:
    """``pair_logodds`` inside the species only, in ``pair_energies_blocked``' form: a list of (kA_s, kB_s) matrices, one per species in
    ascending order of the labels.  Every entry is bit for bit the entry ``pair_logodds`` gives that pairing."""
    mJ, mJA, mJB, Pi, XAf, XBf, N, split, KA, KB = _logodds_args(mJ, mJA, mJB, Pi, XA, XB, q)
    perm_a, perm_b, offA, offB, _ = species_blocks(species_a, species_b)
    if len(perm_a) != KA or len(perm_b) != KB:
        raise ArgumentError(f"species_a / species_b have {len(perm_a)} / {len(perm_b)} labels, XA / XB hold {KA} / {KB} sequences")
    XAs, XBs = np.asfortranarray(XAf[:, perm_a]), np.asfortranarray(XBf[:, perm_b])
    ctx = ctx or default_context()
    L = np.empty(int(np.sum(np.diff(offA).astype(np.int64) * np.diff(offB))), dtype=np.float64)
    ctx.check(ctx.lib.gdca_pair_logodds_blocked(ctx.h, _lib._p(mJ), _lib._p(mJA), _lib._p(mJB), _lib._p(Pi), N, int(q), split, _lib._p(XAs),
                                                KA, _lib._p(XBs), KB, _lib._p(offA), _lib._p(offB), len(offA) - 1, float(information),
                                                _lib._p(L)))
    return _block_views(L, offA, offB)


def assign_blocks(blocks, ctx=None):
    """The minimum-cost one-to-one assignment inside every matrix of ``blocks`` (a list of (kA_s, kB_s) float64 cost matrices: what
    ``pair_energies_blocked`` returns, or any costs), on the device: min(kA_s, kB_s) pairs a species.  Returns ``(match, gap)``, two
    lists with one vector of kA_s entries per species: ``match[s][a]`` the column matched to row a (-1: unmatched), ``gap[s][a]`` the
    least other entry of row a minus the matched one (+inf with one column, 0.0 unmatched, negative where the assignment overrode
    the row's own minimum).  No side may exceed 512."""
    mats = [np.asarray(b, dtype=np.float64) for b in blocks]
    if not mats or any(m.ndim != 2 for m in mats):
        raise ArgumentError("blocks must be a non-empty list of matrices")
    offA = np.concatenate(([0], np.cumsum([m.shape[0] for m in mats]))).astype(np.int32)
    offB = np.concatenate(([0], np.cumsum([m.shape[1] for m in mats]))).astype(np.int32)
    E = np.concatenate([m.ravel(order="F") for m in mats]) if mats else np.empty(0)
    E = np.ascontiguousarray(E, dtype=np.float64)
    KA = int(offA[-1])
    match, gap = np.empty(KA, dtype=np.int32), np.empty(KA, dtype=np.float64)
    ctx = ctx or default_context()
    ctx.check(ctx.lib.gdca_assign_blocks(ctx.h, _lib._p(E), _lib._p(offA), _lib._p(offB), len(mats), _lib._p(match), _lib._p(gap)))
    local = np.where(match >= 0, match - np.repeat(offB[:-1], np.diff(offA)), -1).astype(np.int32)
    cut = offA[1:-1]
    return np.split(local, cut), np.split(gap, cut)


def _mut_what_arg(what) -> int:
    w = str(what).lstrip(":")
    if w == "delta":
        return _lib.MUT_DELTA
    if w == "potential":
        return _lib.MUT_POTENTIAL
    raise ArgumentError(f"invalid what value: {what} (must be either delta or potential)")


def mutation_scan(mJ, Pi, X, q: int = 21, what="delta", ctx=None) -> np.ndarray:
    """D[k, i, b - 1] for every single substitution of the K columns of X (shape (N, K) like Z, symbols 1..q, q = the gap) under the
    Gaussian model (mJ, Pi): ``what="delta"`` the energy change E(x_k with site i set to b) - E(x_k) in the sense of
    ``sequence_energies`` (exactly +0.0 at b = x_i; b = q deletes the residue), ``what="potential"`` the site potential
    V(x; i, c) = sum_{j != i} mJ[r(i,c), r(j,x_j)] + mJ[r(i,c), r(i,c)] / 2 - (mJ Pi)[r(i,c)] (0 for the gap), of which the change is
    the difference V(b) - V(x_i).  Returns a (K, N, q) array.  mJ must be symmetric (its lower triangle is read)."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    w = _mut_what_arg(what)
    Xf = _symbols(X, "X")
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if N < 1 or mJ.shape != (n, n) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites, q = {q}, so mJ must be {n} x {n} and Pi have {n} entries "
                            f"(got {mJ.shape} and {Pi.shape})")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    ctx = ctx or default_context()
    D = np.empty((K, N, int(q)), dtype=np.float64)
    ctx.check(ctx.lib.gdca_mutation_scan(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xf), K, w, _lib._p(D)))
    return D


def _walk_args(N, max_steps, min_gain, mask, gap_target, fill_gaps):
    """the rule's parameters of a greedy walk, checked: (max_steps, min_gain, mask int8 (N,) or None, flags)"""
    if max_steps is None:
        max_steps = min(4 * N, _lib.WALK_MAX_STEPS)
    if not isinstance(max_steps, (int, np.integer)) or not 1 <= max_steps <= _lib.WALK_MAX_STEPS:
        raise ArgumentError(f"invalid max_steps value: {max_steps} (must be an integer between 1 and {_lib.WALK_MAX_STEPS})")
    try:
        min_gain = float(min_gain)
    except (TypeError, ValueError):
        raise ArgumentError(f"invalid min_gain value: {min_gain} (must be a number >= 0)") from None
    if not min_gain >= 0.0:
        raise ArgumentError(f"invalid min_gain value: {min_gain} (must be a number >= 0)")
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != (N,) or not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
            raise ArgumentError(f"mask must be a vector of {N} booleans or integers, one per site")
        mask = np.ascontiguousarray(m != 0, dtype=np.int8)
    return int(max_steps), min_gain, mask, (_lib.WALK_GAP_TARGET if gap_target else 0) | (_lib.WALK_FILL_GAPS if fill_gaps else 0)


def greedy_walk(mJ, Pi, X, q: int = 21, max_steps=None, min_gain: float = 0.0, mask=None, gap_target: bool = False, fill_gaps: bool = False,
                path: bool = False, table: bool = False, ctx=None):
    """Every one of the K columns of X (shape (N, K) like Z, symbols 1..q, q = the gap) descends the energy of the Gaussian model
    (mJ, Pi) greedily: at each step the single substitution with the lowest energy change ``mutation_scan`` would give for the CURRENT
    sequence is taken (ties: the smallest site, then the smallest symbol), until no admissible substitution lowers the energy by more
    than ``min_gain`` or ``max_steps`` (default min(4 N, 65535)) steps are done -- the greedy k-fold mutant, the local minimum the
    sequence drains to, and how far above it the sequence sits.  ``mask``: N booleans, the sites that may change (default all);
    ``gap_target``: a residue may be deleted (the gap is a target); ``fill_gaps``: a gap may receive a residue.  By default residues
    change into residues and gaps stay gaps.

    Returns ``(Xout (N, K) int8, steps (K,) int32, dE_sum (K,))`` -- the final sequences, the steps taken and the sum of the steps'
    energy changes --; with ``path=True`` also ``path (K, max_steps, 2)`` int32, row t = (site, 0-based; symbol, 1..q) of step t and -1
    beyond ``steps[k]``, and ``dE_path (K, max_steps)``, the steps' energy changes and 0 beyond; with ``table=True`` also
    ``V (K, N, q)``, the site potentials as the walk left them (``mutation_scan(.., what="potential")`` of Xout up to the rounding
    of one subtraction and one addition a step).  With ``min_gain = 0`` a pair of moves worth about 1e-16 could in principle alternate
    until max_steps; a min_gain above the table's drift (1e-9 is far above it) rules that out.  mJ must be symmetric (its lower triangle
    is read)."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    Xf = _symbols(X, "X")
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if N < 1 or mJ.shape != (n, n) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites, q = {q}, so mJ must be {n} x {n} and Pi have {n} entries "
                            f"(got {mJ.shape} and {Pi.shape})")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    T, min_gain, m, flags = _walk_args(N, max_steps, min_gain, mask, gap_target, fill_gaps)
    ctx = ctx or default_context()
    out = ctx.walk_outputs(N, K, q, T, path, table)
    opt = lambda a: None if a is None else _lib._p(a)  # noqa: E731
    ctx.check(ctx.lib.gdca_greedy_walk(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xf), K, opt(m), flags, min_gain, T,
                                       *[opt(a) for a in out]))
    return ctx.walk_result(out)


def _sample_args(N, q, beta, burn, stride, n_samples, seed, stream0, mask, gaps):
    """the rule's parameters of the Metropolis chains, checked: (beta, burn, stride, n_samples, seed, stream0, mask int8 (N,) or None,
    flags); burn None: 10 sweeps, stride None: one sweep (a sweep is N proposals)"""
    try:
        beta = float(beta)
    except (TypeError, ValueError):
        raise ArgumentError(f"invalid beta value: {beta} (must be a finite number >= 0)") from None
    if not (beta >= 0.0 and np.isfinite(beta)):
        raise ArgumentError(f"invalid beta value: {beta} (must be a finite number >= 0)")
    burn = 10 * N if burn is None else burn
    stride = N if stride is None else stride
    for v, name, lo in ((burn, "burn", 0), (stride, "stride", 1), (n_samples, "n_samples", 1)):
        if not isinstance(v, (int, np.integer)) or v < lo:
            raise ArgumentError(f"invalid {name} value: {v} (must be an integer >= {lo})")
    if int(burn) + int(n_samples) * int(stride) > 2**31 - 1:
        raise ArgumentError(f"burn + n_samples * stride = {int(burn) + int(n_samples) * int(stride)} proposals are more than 2^31 - 1")
    for v, name in ((seed, "seed"), (stream0, "stream0")):
        if not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2**64:
            raise ArgumentError(f"invalid {name} value: {v} (must be an integer between 0 and 2^64 - 1)")
    if (int(q) if gaps else int(q) - 1) < 2:
        raise ArgumentError(f"q = {q} leaves fewer than two target symbols")
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != (N,) or not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
            raise ArgumentError(f"mask must be a vector of {N} booleans or integers, one per site")
        mask = np.ascontiguousarray(m != 0, dtype=np.int8)
    return beta, int(burn), int(stride), int(n_samples), int(seed), int(stream0), mask, (_lib.SAMPLE_GAPS if gaps else 0)


def sample(mJ, Pi, X, q: int = 21, beta: float = 1.0, burn=None, stride=None, n_samples: int = 1, seed: int = 0, stream0: int = 0, mask=None,
           gaps: bool = False, trace: bool = False, table: bool = False, ctx=None):
    """Metropolis chains under the Gaussian model (mJ, Pi): one chain starts from each of the K columns of X (shape (N, K) like Z,
    symbols 1..q, q = the gap) and draws sequences from exp(-beta E(x)) / Z.  A proposal picks a site that may change and another
    symbol for it, both uniformly; with dE the energy change ``mutation_scan`` would give for the CURRENT sequence it is accepted iff
    ``beta * dE <= -log(u)``, u uniform in (0, 1].  ONE SWEEP IS N PROPOSALS: a chain runs ``burn`` proposals (default 10 N) and then
    returns its state after every ``stride`` (default N) more, ``n_samples`` times.  ``mask``: N booleans, the sites that may change
    (default all); ``gaps``: the gap is a symbol like any other (default: residues change into residues, gaps stay gaps).  The random
    numbers are a function of ``(seed, stream0 + k, proposal)``: chain k of a call is the chain a call with ``stream0 + k`` alone runs.

    Returns ``(Xs (N, n_samples, K) int8, dE_s (K, n_samples), accepted (K,) int32)`` -- ``Xs.reshape(N, -1, order="F")`` is an
    alignment of the n_samples K samples, chain by chain; ``dE_s`` the energy of each sample minus its chain's start's (the running sum
    of the accepted dE); ``accepted`` the accepted proposals of each chain --; with ``trace=True`` also ``thr (K, n_steps)``, the
    thresholds -log(u), and ``moves (K, n_steps)`` int32, the proposal's code ``site * q + symbol`` (both 0-based) if accepted and
    ``-1 - code`` if not; with ``table=True`` also ``V (K, N, q)``, the site potentials as the chain left them.  mJ must be symmetric
    (its lower triangle is read)."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    Xf = _symbols(X, "X")
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if N < 1 or mJ.shape != (n, n) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites, q = {q}, so mJ must be {n} x {n} and Pi have {n} entries "
                            f"(got {mJ.shape} and {Pi.shape})")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    beta, burn, stride, S, seed, stream0, m, flags = _sample_args(N, q, beta, burn, stride, n_samples, seed, stream0, mask, gaps)
    ctx = ctx or default_context()
    out = ctx.sample_outputs(N, K, q, burn, stride, S, trace, table)
    opt = lambda a: None if a is None else _lib._p(a)  # noqa: E731
    ctx.check(ctx.lib.gdca_sample(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xf), K, opt(m), flags, beta, seed, stream0, burn, stride,
                                  S, *[opt(a) for a in out]))
    return ctx.sample_result(out)


def _temper_args(N, betas, swap_every, burn, stride):
    """the ladder and the round schedule of the replica-exchange chains, checked: (betas f64 (R,), swap_every); swap_every None: one sweep"""
    try:
        b = np.asarray(betas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ArgumentError(f"invalid betas: {betas} (must be 1 to {_lib.TEMPER_MAX} finite numbers >= 0, the target first)") from None
    if not 1 <= b.size <= _lib.TEMPER_MAX:
        raise ArgumentError(f"invalid betas: {b.size} replicas (must be 1 to {_lib.TEMPER_MAX} finite numbers >= 0, the target first)")
    if not np.all(np.isfinite(b) & (b >= 0.0)):
        raise ArgumentError(f"invalid betas: {betas} (every beta must be a finite number >= 0)")
    swap_every = N if swap_every is None else swap_every
    if not isinstance(swap_every, (int, np.integer)) or swap_every < 1:
        raise ArgumentError(f"invalid swap_every value: {swap_every} (must be an integer >= 1)")
    if burn % int(swap_every) or stride % int(swap_every):
        raise ArgumentError(f"invalid swap_every value: {swap_every} (must divide burn = {burn} and stride = {stride})")
    return np.ascontiguousarray(b), int(swap_every)


def sample_tempered(mJ, Pi, X, q: int = 21, betas=(1.0,), swap_every=None, burn=None, stride=None, n_samples: int = 1, seed: int = 0,
                    stream0: int = 0, mask=None, gaps: bool = False, slot0=None, trace: bool = False, ctx=None):
    """Replica-exchange (parallel tempering) Metropolis chains under the Gaussian model (mJ, Pi).  Every one of K chains runs
    R = len(betas) replicas; a replica is a chain of ``sample`` on a stream of its own (``stream0 + k R + r``) at the inverse
    temperature ``betas[slot]`` of the slot it holds, accepting a proposal iff ``beta * dE <= -log(u)``.  After every ``swap_every``
    proposals (default N, one sweep; it must divide ``burn`` and ``stride``) round e lets the holders a, b of the slots p, p + 1 with
    p % 2 == e % 2 exchange their slots iff ``(betas[p] - betas[p + 1]) * (E_b - E_a) <= -log(u)``.  ``betas[0]`` is the target
    temperature: only the holder of slot 0 is sampled, after ``burn`` proposals (default 10 N) and every ``stride`` (default N) more.
    X is (N, K) -- every replica of chain k starts at X[:, k] -- or (N, R, K); ``slot0`` (K, R): the slot every replica holds at the
    start (default: replica r holds slot r).  ``mask``, ``gaps``, ``seed`` as ``sample``.

    Returns ``(Xs (N, n_samples, K) int8, E_s (K, n_samples), accepted (K, R) int32, swaps (K, R - 1) int32, Xr_out (N, R, K) int8,
    slot_out (K, R) int32)``: the samples, their energies, the accepted proposals by SLOT, the accepted swaps by pair, and the final
    states and slots (hand them back as X and slot0 to continue); with ``trace=True`` also ``thr, moves (K, R, n_steps)``, ``swap_thr
    (K, R - 1, n_rounds)`` and ``slot_path (K, R, n_rounds)``."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    Xa = np.asarray(X)
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    if Xa.ndim not in (2, 3):
        raise ArgumentError("X must be an (N, K) or an (N, R, K) array of symbols")
    N, K = Xa.shape[0], Xa.shape[-1]
    n = N * (int(q) - 1)
    if N < 1 or mJ.shape != (n, n) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites, q = {q}, so mJ must be {n} x {n} and Pi have {n} entries "
                            f"(got {mJ.shape} and {Pi.shape})")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    _, burn, stride, S, seed, stream0, m, flags = _sample_args(N, q, 1.0, burn, stride, n_samples, seed, stream0, mask, gaps)
    b, swap_every = _temper_args(N, betas, swap_every, burn, stride)
    R = b.size
    if Xa.ndim == 3 and Xa.shape[1] != R:
        raise ArgumentError(f"incompatible sizes: X has {Xa.shape[1]} replicas a chain, betas has {R}")
    Xr = _symbols(np.repeat(Xa[:, None, :], R, axis=1).reshape(N, R * K, order="F") if Xa.ndim == 2 else Xa.reshape(N, R * K, order="F"), "X")
    s0 = None
    if slot0 is not None:
        s0 = np.asarray(slot0)
        if s0.shape != (K, R) or not np.issubdtype(s0.dtype, np.integer) or not np.all(np.sort(s0, axis=1) == np.arange(R)):
            raise ArgumentError(f"slot0 must be {K} x {R} integers, every row a permutation of 0 .. {R - 1}")
        s0 = np.ascontiguousarray(s0, dtype=np.int32)
    ctx = ctx or default_context()
    out = ctx.tempered_outputs(N, K, R, swap_every, burn, stride, S, trace)
    opt = lambda a: None if a is None or a.size == 0 else _lib._p(a)  # noqa: E731
    ptrs = [opt(a) for a in out]
    ptrs[3] = ctx._swaps_arg(out[3])
    ctx.check(ctx.lib.gdca_sample_tempered(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xr), opt(s0), K, R, _lib._p(b), opt(m), flags,
                                           seed, stream0, swap_every, burn, stride, S, *ptrs))
    return tuple(a for a in out if a is not None)


def _ladder_arg(betas, n_stages, beta):
    """the ladder of annealed importance sampling, checked: f64 (L + 1,), betas[0] == 0; betas None: np.linspace(0, beta, n_stages + 1)"""
    if betas is None:
        if not isinstance(n_stages, (int, np.integer)) or n_stages < 1:
            raise ArgumentError(f"invalid n_stages value: {n_stages} (must be an integer >= 1)")
        try:
            beta = float(beta)
        except (TypeError, ValueError):
            raise ArgumentError(f"invalid beta value: {beta} (must be a finite number >= 0)") from None
        if not (beta >= 0.0 and np.isfinite(beta)):
            raise ArgumentError(f"invalid beta value: {beta} (must be a finite number >= 0)")
        return np.linspace(0.0, beta, int(n_stages) + 1)
    try:
        b = np.asarray(betas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ArgumentError(f"invalid betas: {betas} (must be at least two finite numbers >= 0, the first 0)") from None
    if b.size < 2:
        raise ArgumentError(f"invalid betas: {b.size} values (must be at least two finite numbers >= 0, the first 0)")
    if not np.all(np.isfinite(b) & (b >= 0.0)):
        raise ArgumentError(f"invalid betas: {betas} (every beta must be a finite number >= 0)")
    if b[0] != 0.0:
        raise ArgumentError(f"invalid betas: betas[0] = {b[0]} (must be 0: the chains start from the uniform distribution)")
    return np.ascontiguousarray(b)


def _state_space(N, q, x, mask, gaps):
    """the state space of annealed importance sampling, checked: (x int8 (N,) or None, mask int8 (N,) or None, free (N,) bool)"""
    if x is None:
        if mask is not None:
            raise ArgumentError("mask needs a template x (the symbols of the sites that do not move)")
        return None, None, np.ones(N, dtype=bool)
    xa = np.asarray(x)
    if xa.shape != (N,) or not np.issubdtype(xa.dtype, np.integer) or (xa.size and (xa.min() < 1 or xa.max() > q)):
        raise ArgumentError(f"x must be a vector of {N} integer symbols between 1 and q = {q}")
    xa = np.ascontiguousarray(xa, dtype=np.int8)
    free = np.ones(N, dtype=bool) if gaps else xa != q
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != (N,) or not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
            raise ArgumentError(f"mask must be a vector of {N} booleans or integers, one per site")
        mask = np.ascontiguousarray(m != 0, dtype=np.int8)
        free &= mask != 0
    return xa, mask, free


def log_partition(mJ, Pi, q: int = 21, betas=None, n_stages: int = 100, beta: float = 1.0, sweep=None, K: int = 1024, x=None, mask=None,
                  gaps: bool = False, seed: int = 0, stream0: int = 0, trace: bool = False, ctx=None):
    """log Z(beta) = log sum_x exp(-beta E(x)) of the model (mJ, Pi) read as a Potts model -- a fit of ``gDCA_bm`` or ``gDCA_plm`` as
    (W, zeros), or the Gaussian fit as the chains read it -- by annealed importance sampling (Neal 2001).  The sum runs over the state
    space of the template ``x`` (N symbols 1..q): the sites ``mask`` lets change (default all) take every residue, or with ``gaps=True``
    every symbol; without it the template's gaps stay gaps; every other site keeps the template's symbol.  ``x=None`` (no mask then):
    every site is free.  K chains start at uniform draws from that space and run ``sweep`` Metropolis proposals (default one sweep,
    the number of free sites) at each of the inverse temperatures ``betas[1:]``, ``betas[0] == 0`` (default
    ``np.linspace(0, beta, n_stages + 1)``); chain k's weight is the product of exp(-(betas[l] - betas[l-1]) E) over the states it
    stood in ahead of every stage, and |Omega| mean(w) estimates Z(betas[-1]) without bias for any ladder and any sweep.

    Returns ``(logZ, ess, logw (K,))``: the estimate, the effective sample size (sum w)^2 / sum w^2 in [1, K] -- an ess far below K
    says the ladder is too coarse or the sweeps too short -- and the chains' log-weights; with ``trace=True`` also ``E_end (K,)``,
    ``X0 (N, K)`` and ``Xout (N, K)`` int8 (the starts and the final states: with logw a weighted sample of the target),
    ``accepted (K,)`` int32, ``thr`` and ``moves (K, n_steps)`` as ``sample`` returns them.  mJ must be symmetric (its lower triangle
    is read)."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = Pi.shape[0] if Pi.ndim == 1 else -1
    if n < 1 or n % (int(q) - 1) or mJ.shape != (n, n):
        raise ArgumentError(f"incompatible sizes: q = {q}, mJ {mJ.shape}, Pi {Pi.shape} (mJ must be n x n, Pi have n = N (q - 1) entries)")
    N = n // (int(q) - 1)
    b = _ladder_arg(betas, n_stages, beta)
    if not isinstance(K, (int, np.integer)) or K < 1:
        raise ArgumentError(f"invalid K value: {K} (must be an integer >= 1)")
    xa, m, free = _state_space(N, int(q), x, mask, gaps)
    sweep = max(int(free.sum()), 1) if sweep is None else sweep
    if not isinstance(sweep, (int, np.integer)) or sweep < 1:
        raise ArgumentError(f"invalid sweep value: {sweep} (must be an integer >= 1)")
    L = b.size - 1
    if L * int(sweep) > 2**31 - 1:
        raise ArgumentError(f"invalid sweep value: {L} stages of {sweep} proposals are more than 2^31 - 1")
    _, _, _, _, seed, stream0, _, flags = _sample_args(N, q, 1.0, 0, 1, 1, seed, stream0, None, gaps)
    ctx = ctx or default_context()
    out = ctx.log_partition_outputs(N, int(K), L * int(sweep), trace)
    opt = lambda a: None if a is None else _lib._p(a)  # noqa: E731
    ctx.check(ctx.lib.gdca_log_partition(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), opt(xa), opt(m), flags, _lib._p(b), L, int(sweep), int(K),
                                         seed, stream0, *[opt(a) for a in out]))
    return (float(out[0][0]), float(out[0][1]), out[1]) + tuple(a for a in out[2:] if a is not None)


def potts_loglik(mJ, Pi, X, q: int = 21, **kw):
    """The log-likelihood of the K columns of X (shape (N, K), symbols 1..q) under the Potts reading of (mJ, Pi):
    ``L[k] = -beta E(x_k) - logZ`` with E from ``sequence_energies`` and (logZ, ess) from ``log_partition(mJ, Pi, q, **kw)`` at its
    target temperature (default beta = 1: ``L = -E - logZ``) -- what makes a held-out score of a ``gDCA_plm`` or a ``gDCA_bm`` fit
    comparable across fits.  Every sequence must lie in the state space logZ sums over: no gap without ``gaps=True`` (or outside the
    template's gaps), and the template's symbol at every site that does not move.  Returns ``(L (K,), logZ, ess)``."""
    if kw.get("trace"):
        raise ArgumentError("trace is not an argument of potts_loglik (log_partition returns the traces)")
    Xf = _symbols(X, "X")
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or not 2 <= q <= 31:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    if Xf.min() < 1 or Xf.max() > q:
        raise ArgumentError("X must hold integer symbols between 1 and q")
    b = _ladder_arg(kw.get("betas"), kw.get("n_stages", 100), kw.get("beta", 1.0))
    xa, _, free = _state_space(N, int(q), kw.get("x"), kw.get("mask"), bool(kw.get("gaps", False)))
    if not kw.get("gaps", False) and np.any(Xf[free] == q):
        raise ArgumentError("X holds a sequence outside the state space: a gap at a free site (gaps=True makes the gap a symbol)")
    if xa is not None and np.any(Xf[~free] != xa[~free, None]):
        raise ArgumentError("X holds a sequence outside the state space: it differs from the template x at a site that does not move")
    logZ, ess, _ = log_partition(mJ, Pi, q, **kw)
    E = sequence_energies(mJ, Pi, Xf, q, ctx=kw.get("ctx"))
    return -(b[-1] * E) - logZ, logZ, ess


def potts_independent(Pi, N: int, q: int = 21):
    """The independent-site Potts model (W, zeros) of the single-site frequencies Pi (n = N (q - 1) entries, all and every site's gap
    frequency 1 - sum positive): couplings zero, W[r, r] = -2 log(Pi[r] / Pi_gap(site)) -- the start of ``gDCA_bm(init="independent")``."""
    P = np.asarray(Pi, dtype=np.float64).reshape(int(N), int(q) - 1)
    return np.asfortranarray(np.diag((-2.0 * np.log(P / (1.0 - P.sum(axis=1))[:, None])).ravel()))


def potts_from_gaussian(mJ, Pi, q: int = 21, ctx=None):
    """The Gaussian model (mJ, Pi) as a Potts model in mJ's layout (gdca_potts_from_gaussian): returns W (n, n) with the couplings of
    mJ in its off-diagonal blocks, W[r, r] = mJ[r, r] - 2 (mJ Pi)[r] and +0.0 elsewhere in a diagonal block.  (W, zeros) is a model
    every read-out of this module takes in the place of (mJ, Pi): the same energy differences, and what ``bm_learn`` refines."""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    n = Pi.shape[0] if Pi.ndim == 1 else -1
    if not isinstance(q, (int, np.integer)) or not 2 <= q <= 31 or n < 1 or n % (int(q) - 1) or mJ.shape != (n, n):
        raise ArgumentError(f"incompatible sizes: q = {q}, mJ {mJ.shape}, Pi {Pi.shape} (mJ must be n x n, Pi have n = N (q - 1) entries)")
    ctx = ctx or default_context()
    W = np.empty((n, n), dtype=np.float64, order="F")
    ctx.check(ctx.lib.gdca_potts_from_gaussian(ctx.h, _lib._p(mJ), _lib._p(Pi), n // (int(q) - 1), int(q), _lib._p(W)))
    return W


def bm_learn(W, Pi_d, Pij_d, X, n_iter: int, q: int = 21, eta: float = 1.0, lam: float = 0.0, beta: float = 1.0, burn=None, stride=None,
             n_samples: int = 1, seed: int = 0, iter0: int = 0, mask=None, gaps: bool = True, ctx=None, betas=None, swap_every=None,
             slot0=None):
    """n_iter iterations of Boltzmann-machine learning on host arrays (gdca_bm_learn): the Potts model W (n, n) -- from
    ``potts_from_gaussian`` or ``potts_independent`` -- is moved towards the frequencies (Pi_d, Pij_d) by sampling K persistent
    Metropolis chains from the columns of X (N, K), tallying the K n_samples samples and adding eta times the difference of the model's
    and the data's frequencies; ``lam`` is an L2 penalty on the couplings.  ``burn`` (default 10 N), ``stride`` (default N), ``mask``,
    ``gaps`` (default True: the gap is a symbol like any other) as ``sample``.  Returns (W, X, trace (n_iter, 4)): new arrays; trace
    holds max |Pi_m - Pi_d|, max |c_m - c_d|, the Pearson correlation of the connected correlations and the acceptance rate of every
    iteration.  A later call with ``iter0 + n_iter`` continues the same run bit for bit.

    ``betas`` (a ladder of inverse temperatures, the target first; ``beta`` is then not used): replica-exchange chains in the place of
    the plain ones (``devops.bm_learn_tempered_dev``, driven from Python; ``swap_every`` default N).  X is (N, K) -- every replica of
    chain k starts at X[:, k] -- or (N, R, K) with ``slot0`` (K, R) to continue a run.  Returns (W, Xr (N, R, K), trace, slot (K, R),
    swap_rates (n_iter, R - 1)); with ``betas=(beta,)`` W, Xr[:, 0, :] and trace are the plain loop's bit for bit."""
    W = np.array(W, dtype=np.float64, order="F")
    Pi_d = np.ascontiguousarray(Pi_d, dtype=np.float64)
    Pij_d = np.ascontiguousarray(Pij_d, dtype=np.float64)
    Xa = np.asarray(X)
    R = None
    if betas is not None:
        if Xa.ndim not in (2, 3):
            raise ArgumentError("X must be an (N, K) or an (N, R, K) array of symbols")
        R = len(np.atleast_1d(np.asarray(betas, dtype=object)))
        if Xa.ndim == 3 and Xa.shape[1] != R:
            raise ArgumentError(f"incompatible sizes: X has {Xa.shape[1]} replicas a chain, betas has {R}")
        Xr = np.repeat(Xa[:, None, :], R, axis=1) if Xa.ndim == 2 else Xa
        Xa = Xr.reshape(Xr.shape[0], -1, order="F")[:, ::R] if R else Xa  # (one column a chain: the checks below)
    Xf = np.array(_symbols(Xa, "X"), dtype=np.int8, order="F")
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or not 2 <= q <= 31:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    n = N * (int(q) - 1)
    if N < 1 or W.shape != (n, n) or Pij_d.shape != (n, n) or Pi_d.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites, q = {q}, so W and Pij_d must be {n} x {n} and Pi_d have {n} entries")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    for v, name in ((eta, "eta"), (lam, "lam")):
        if not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or (name == "eta" and v == 0):
            raise ArgumentError(f"invalid {name} value: {v}")
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ArgumentError(f"invalid n_iter value: {n_iter} (must be an integer >= 1)")
    beta, burn, stride, S, seed, iter0, m, flags = _sample_args(N, q, beta, burn, stride, n_samples, seed, iter0, mask, gaps)
    ctx = ctx or default_context()
    if betas is not None:
        from . import devops

        b, every = _temper_args(N, betas, swap_every, burn, stride)
        Xrf = _symbols(Xr.reshape(N, R * K, order="F"), "X")
        s0 = None
        if slot0 is not None:
            s0 = np.asarray(slot0)
            if s0.shape != (K, R) or not np.issubdtype(s0.dtype, np.integer) or not np.all(np.sort(s0, axis=1) == np.arange(R)):
                raise ArgumentError(f"slot0 must be {K} x {R} integers, every row a permutation of 0 .. {R - 1}")
        up = lambda a: _lib.DeviceBuffer.from_array(ctx, a)  # noqa: E731
        dW, dPi, dPij, dXr = up(W), up(Pi_d), up(Pij_d), up(Xrf)
        dslot = None if s0 is None else up(np.ascontiguousarray(s0, dtype=np.int32))
        dmask = None if m is None else up(m)
        dXo, dso, trace, rates = devops.bm_learn_tempered_dev(ctx, dW, dPi, dPij, N, int(q), dXr, dslot, K, b, int(n_iter), burn, stride, S,
                                                              float(eta), float(lam), every, seed, iter0, dmask, flags)
        out = (dW.download((n, n)), dXo.download((N, R, K), np.int8), trace, dso.download((K, R), np.int32, order="C"), rates)
        for d in (dW, dPi, dPij, dXr, dslot, dmask, dXo, dso):
            if d is not None:
                d.free()
        return out
    trace = np.empty((int(n_iter), 4), dtype=np.float64)
    ctx.check(ctx.lib.gdca_bm_learn(ctx.h, _lib._p(W), _lib._p(Pi_d), _lib._p(Pij_d), N, int(q), _lib._p(Xf), K,
                                    None if m is None else _lib._p(m), flags, beta, seed, iter0, int(n_iter), burn, stride, S, float(eta),
                                    float(lam), _lib._p(trace), None))
    return W, Xf, trace


def _plm_args(W, Z, q, w=None, Meff=None):
    """the model, the sequences and the weights of the pseudo-likelihood operators, checked: (W, Zf, N, M, w)"""
    W = np.asfortranarray(W, dtype=np.float64)
    Zf = _symbols(Z, "Z", "an N x M")
    N, M = Zf.shape
    if not isinstance(q, (int, np.integer)) or not 2 <= q <= 31:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    n = N * (int(q) - 1)
    if N < 1 or M < 1 or W.shape != (n, n):
        raise ArgumentError(f"incompatible sizes: Z has N = {N} sites, q = {q}, so W must be {n} x {n}")
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (M,) or not isinstance(Meff, (int, float, np.integer, np.floating)) or not Meff > 0:
            raise ArgumentError(f"incompatible weights: w must have M = {M} entries and Meff be positive")
    return W, Zf, N, M, w


def plm_conditionals(W, Z, q: int = 21, ctx=None):
    """The conditionals of the sequences Z (N, M) under the Potts model (W, zeros) on host arrays (gdca_plm_conditionals): returns
    (p (M, N, q): p[k, i, c - 1] = P(x_i = c | the rest of sequence k), the gap last; nll_k (M,): -sum_i log P(x_ki | rest))."""
    W, Zf, N, M, _ = _plm_args(W, Z, q)
    ctx = ctx or default_context()
    p, nll_k = np.empty((M, N, int(q)), dtype=np.float64), np.empty(M, dtype=np.float64)
    ctx.check(ctx.lib.gdca_plm_conditionals(ctx.h, _lib._p(W), _lib._p(Zf), N, M, int(q), _lib._p(p), _lib._p(nll_k)))
    return p, nll_k


def plm_tallies(W, Z, w, Meff: float, q: int = 21, ctx=None):
    """The conditional tallies of the pseudo-likelihood on host arrays (gdca_plm_tallies): returns (Pi_c (n,), Pij_c (n, n), nll) of
    the sequences Z (N, M) with the weights w (M,) and Meff (``compute_weights``'s) under (W, zeros).  With (Pi_d, Pij_d) of
    ``compute_weighted_frequencies``, 2 (Pij_c - Pij_d) is the gradient of the log pseudo-likelihood by the couplings and
    1/2 (Pi_c - Pi_d) by W's diagonal."""
    W, Zf, N, M, w = _plm_args(W, Z, q, w, Meff)
    n = N * (int(q) - 1)
    ctx = ctx or default_context()
    Pi_c, Pij_c, nll = np.empty(n, dtype=np.float64), np.empty((n, n), dtype=np.float64, order="F"), np.empty(1, dtype=np.float64)
    ctx.check(ctx.lib.gdca_plm_tallies(ctx.h, _lib._p(W), _lib._p(Zf), _lib._p(w), float(Meff), N, M, int(q), _lib._p(Pi_c), _lib._p(Pij_c),
                                       _lib._p(nll)))
    return Pi_c, Pij_c, float(nll[0])


def plm_learn(W, Z, w, Meff: float, Pi_d, Pij_d, n_iter: int, q: int = 21, eta=None, lam: float = 0.01, ctx=None):
    """n_iter iterations of pseudo-likelihood ascent on host arrays (gdca_plm_learn): W (n, n) is moved by ``bm_learn``'s step with the
    conditional tallies of Z (N, M), w, Meff in the place of the sampler's.  ``eta=None`` is 1 / (N + 2 lam).  Returns (W, trace
    (n_iter, 4)): new arrays; trace holds max |Pi_c - Pi_d|, max |c_c - c_d|, the Pearson correlation of the connected correlations and
    nll per iteration.  A later call continues the same run bit for bit."""
    W, Zf, N, M, w = _plm_args(W, Z, q, w, Meff)
    W = np.array(W, dtype=np.float64, order="F")
    n = N * (int(q) - 1)
    Pi_d = np.ascontiguousarray(Pi_d, dtype=np.float64)
    Pij_d = np.ascontiguousarray(Pij_d, dtype=np.float64)
    if Pij_d.shape != (n, n) or Pi_d.shape != (n,):
        raise ArgumentError(f"incompatible sizes: Pij_d must be {n} x {n} and Pi_d have {n} entries")
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ArgumentError(f"invalid n_iter value: {n_iter} (must be an integer >= 1)")
    eta = 1.0 / (N + 2.0 * float(lam)) if eta is None else eta
    for v, name in ((eta, "eta"), (lam, "lam")):
        if not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or (name == "eta" and v == 0):
            raise ArgumentError(f"invalid {name} value: {v}")
    ctx = ctx or default_context()
    trace = np.empty((int(n_iter), 4), dtype=np.float64)
    ctx.check(ctx.lib.gdca_plm_learn(ctx.h, _lib._p(W), _lib._p(Zf), _lib._p(w), float(Meff), _lib._p(Pi_d), _lib._p(Pij_d), N, M, int(q),
                                     int(n_iter), float(eta), float(lam), _lib._p(trace)))
    return W, trace


def _double_model_args(mJ, Pi, X, q):
    """the model and the sequences of the double-mutant operators, checked: (mJ, Pi, Xf, N, K)"""
    mJ = np.ascontiguousarray(mJ, dtype=np.float64)
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    Xf = _symbols(X, "X")
    N, K = Xf.shape
    if not isinstance(q, (int, np.integer)) or q < 2:
        raise ArgumentError(f"invalid q value: {q} (must be an integer between 2 and 31)")
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (int(q) - 1)
    if N < 2 or mJ.shape != (n, n) or Pi.shape != (n,):
        raise ArgumentError(f"incompatible sizes: X has N = {N} sites (at least 2 are needed), q = {q}, so mJ must be {n} x {n} and Pi "
                            f"have {n} entries (got {mJ.shape} and {Pi.shape})")
    if K < 1:
        raise ArgumentError("X holds no sequence")
    return mJ, Pi, Xf, N, K


def decode_double_code(code, q: int):
    """code = (b - 1) + q (c - 1) of a double-mutant map -> (sub_i, sub_j) int8, the symbols b and c; 0 where code < 0 (the diagonal)"""
    code = np.asarray(code)
    ok = code >= 0
    return (np.where(ok, code % int(q) + 1, 0).astype(np.int8), np.where(ok, code // int(q) + 1, 0).astype(np.int8))


def double_mutant_scan(mJ, Pi, X, q: int = 21, ctx=None):
    """The double-mutant landscape of the K columns of X (shape (N, K) like Z, symbols 1..q, q = the gap) under the Gaussian model
    (mJ, Pi), one entry a site pair: ``(ddE_min, sub_i, sub_j, epistasis)``, each of shape (K, N, N) and indexed [k, i, j].
    ddE_min[k, i, j] is the lowest energy change, in the sense of ``sequence_energies``, over the true double substitutions of sites i and
    j (both symbols changed; the gap q is a target, "delete"), sub_i / sub_j (int8) the symbols it puts at site i and at site j, and
    epistasis[k, i, j] = sqrt(sum over all targets of eps^2) with eps the part of a double mutant's energy change that is not the sum of
    the two single changes ``mutation_scan`` gives.  ddE_min and epistasis are symmetric; the diagonal holds 0.  No mutant is written
    down.  mJ must be symmetric (its lower triangle is read)."""
    mJ, Pi, Xf, N, K = _double_model_args(mJ, Pi, X, q)
    ctx = ctx or default_context()
    Emin, code, epi = (np.empty((K, N, N), dtype=np.float64), np.empty((K, N, N), dtype=np.int32), np.empty((K, N, N), dtype=np.float64))
    ctx.check(ctx.lib.gdca_double_mutant_scan(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xf), K, _lib._p(Emin), _lib._p(code),
                                              _lib._p(epi)))
    # (the library's [i + N (j + N k)] is [k, j, i] here: Emin and epi are symmetric, the transposed code names sub_i first)
    sub_i, sub_j = decode_double_code(code.transpose(0, 2, 1), q)
    return Emin, sub_i, sub_j, epi


def _mutations_arg(muts) -> np.ndarray:
    """(L, 5) records (k, i, b, j, c) -> int32, one record after the other in memory (the library's 5 x L column-major)"""
    m = np.asarray(muts)
    if m.ndim != 2 or m.shape[1] != 5 or not np.issubdtype(m.dtype, np.integer):
        raise ArgumentError("mutations must be an (L, 5) integer array of records (k, i, b, j, c)")
    if m.shape[0] < 1:
        raise ArgumentError("mutations holds no record")
    if m.size and (m.min() < np.iinfo(np.int32).min or m.max() > np.iinfo(np.int32).max):
        raise ArgumentError("mutations holds a value beyond int32")
    return np.ascontiguousarray(m, dtype=np.int32)


def double_mutant_energies(mJ, Pi, X, muts, q: int = 21, ctx=None) -> np.ndarray:
    """The energy change of the listed double mutants: ``muts`` is an (L, 5) integer array of records (k, i, b, j, c) -- sequence k
    (a column of X), 0-based sites i != j, the symbols b (put at i) and c (put at j) in 1..q -- and the result has L entries, E(x_k with
    i -> b, j -> c) - E(x_k) in the sense of ``sequence_energies``.  Which substitution is named first does not matter; a target equal to
    the sequence's own symbol is allowed (the result is then the single change of the other site)."""
    mJ, Pi, Xf, N, K = _double_model_args(mJ, Pi, X, q)
    m = _mutations_arg(muts)
    ctx = ctx or default_context()
    out = np.empty(m.shape[0], dtype=np.float64)
    ctx.check(ctx.lib.gdca_double_mutants(ctx.h, _lib._p(mJ), _lib._p(Pi), N, int(q), _lib._p(Xf), K, _lib._p(m), m.shape[0], _lib._p(out)))
    return out


def printrank(io, R: Sequence[Tuple[int, int, float]] = None):
    """printrank(io, R) / printrank(filename, R): one "%i %i %e" line per entry
    (src/GaussDCA.jl:67-74).  printrank(R) alone writes to stdout (the reference's one-argument
    method references the undefined STDOUT and throws; here it works)."""
    import sys

    if R is None:
        io, R = sys.stdout, io
    if isinstance(io, (str, bytes)):
        lib = _lib.load()
        if isinstance(R, Ranking):
            ii, jj, sc = (np.ascontiguousarray(R.i, dtype=np.int32), np.ascontiguousarray(R.j, dtype=np.int32),
                          np.ascontiguousarray(R.score, dtype=np.float64))
        else:
            ii = np.asarray([r[0] for r in R], dtype=np.int32)
            jj = np.asarray([r[1] for r in R], dtype=np.int32)
            sc = np.asarray([r[2] for r in R], dtype=np.float64)
        path = io if isinstance(io, bytes) else io.encode()
        if lib.gdca_write_rank(path, _lib._p(ii), _lib._p(jj), _lib._p(sc), len(R)) != 0:
            raise OSError(f"cannot write {io}")
        return None
    for (i, j, x) in R:
        io.write("%i %i %e\n" % (i, j, x))
