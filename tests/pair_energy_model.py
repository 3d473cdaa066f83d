"""The pair-energy rule in numpy (the checker of tests/test_pair_energy_cpu.py and tests/test_gpu_pair_energy.py).

An alignment of concatenated pairs: sites 0 .. split - 1 are protein A, the rest protein B.  With the one-hot x = xA (+) xB of
tests/energy_model.py, g = mJ Pi and c0 = Pi' g, the energy of a concatenation splits exactly:

    E(a (+) b) = E(a (+) gaps) + E(gaps (+) b) - c0 / 2 + R(a, b)
    R(a, b)    = sum_{i in A, j in B, neither a gap} mJ[r(j), r(i)],   r(i) = i s + a_i - 1

(the quadratic form's cross terms appear twice with the factor 1/2, so each pair (i, j) once; each marginal energy carries c0 / 2).

  coupling_gather  R and B_R = the sum of the terms' absolute values, both accumulated in np.longdouble;
  pair_energy      the composition above on energy_model.energies_gather, with the bound of the concatenation.

Bounds, derived: any order of the N_A N_B terms of R errs by at most (N_A N_B - 1) u B_R to first order; the factor 2 covers the
second-order terms as in energy_model.order_bound:  |R - R_ref| <= 2 N_A N_B u B_R.  The energy: order_bound(N, q, B_cat + |c0|),
B_cat that of the concatenation (all its terms appear in the composition) and |c0| for the two extra appearances of c0 / 2.
XA is (split, K_A), XB is (N - split, K_B): sequences are columns."""
import numpy as np

import energy_model as em


def _rows(col, q, site0=0):
    """global one-hot rows of the non-gap sites of one half"""
    col = np.asarray(col).astype(np.int64)
    sites = np.nonzero((col >= 1) & (col < q))[0]
    return (sites + site0) * (q - 1) + col[sites] - 1


def coupling_gather(mJ, XA, XB, q):
    """-> (R float64 (K_A, K_B) rounded once from the longdouble sums, B_R float64 (K_A, K_B))"""
    XA, XB = np.asarray(XA), np.asarray(XB)
    split, KA = XA.shape
    NB, KB = XB.shape
    s = q - 1
    nA, nB = split * s, NB * s
    L = np.asarray(mJ)[nA:, :nA].astype(np.longdouble)  # the only block the cross terms touch: rows of B, columns of A
    La = np.abs(L)
    # the rows of the block every b selects; a gap selects the appended zero at index nB
    xb = XB.astype(np.int64)
    IB = np.where((xb >= 1) & (xb < q), np.arange(NB)[:, None] * s + xb - 1, nB).T  # (K_B, N_B)
    R = np.zeros((KA, KB))
    B = np.zeros((KA, KB))
    zero = np.zeros(1, dtype=np.longdouble)
    for a in range(KA):
        ra = _rows(XA[:, a], q)
        if not ra.size:
            continue
        # (T[row] = sum_i L[row, r_a(i)] first, then the rows b selects: one order of the double sum, in longdouble)
        Ta = np.concatenate([L[:, ra].sum(axis=1, dtype=np.longdouble), zero])
        Tabs = np.concatenate([La[:, ra].sum(axis=1, dtype=np.longdouble), zero])
        R[a] = Ta[IB].sum(axis=1, dtype=np.longdouble).astype(np.float64)
        B[a] = Tabs[IB].sum(axis=1, dtype=np.longdouble).astype(np.float64)
    return R, B


def coupling_bound(NA, NB, B_R):
    return 2.0 * NA * NB * em.U * np.asarray(B_R)


def concatenations(XA, XB, q=None):
    """(N, K_A K_B) int8, column a + K_A * b = a (+) b"""
    XA, XB = np.asarray(XA), np.asarray(XB)
    KA, KB = XA.shape[1], XB.shape[1]
    top = np.tile(XA, (1, KB))
    bot = np.repeat(XB, KA, axis=1)
    return np.asfortranarray(np.concatenate([top, bot], axis=0).astype(np.int8))


def padded(XA, XB, q):
    """a (+) gaps (N, K_A) and gaps (+) b (N, K_B)"""
    XA, XB = np.asarray(XA), np.asarray(XB)
    PA = np.concatenate([XA, np.full((XB.shape[0], XA.shape[1]), q, dtype=XA.dtype)], axis=0)
    PB = np.concatenate([np.full((XA.shape[0], XB.shape[1]), q, dtype=XB.dtype), XB], axis=0)
    return PA, PB


def pair_energy(mJ, Pi, XA, XB, q):
    """The composition -> (E (K_A, K_B), bound (K_A, K_B), c0, EA, EB): bound = order_bound(N, q, B_cat + |c0|) with B_cat the
    sum of the absolute terms of the concatenation: those of both marginals, minus the |c0| / 2 they share, plus the cross terms."""
    XA, XB = np.asarray(XA), np.asarray(XB)
    N = XA.shape[0] + XB.shape[0]
    PA, PB = padded(XA, XB, q)
    EA, BA, c0 = em.energies_gather(mJ, Pi, PA, q)
    EB, BB, _ = em.energies_gather(mJ, Pi, PB, q)
    R, BR = coupling_gather(mJ, XA, XB, q)
    E = (EA[:, None] + EB[None, :] - c0 / 2) + R
    B_cat = BA[:, None] + BB[None, :] - abs(c0) / 2 + BR
    return E, em.order_bound(N, q, B_cat + abs(c0)), c0, EA, EB


def mixed_halves(rng, Zo, q, split, KA, KB, shift=0):
    """XA (split, KA), XB (N - split, KB) int8, column-major: column j is, by (j + shift) % 4: all gaps, a sequence without gaps, a
    uniformly random one (gaps included), that half of a member of the family (as test_gpu_energy.mixed_sequences)"""
    M, N = Zo.shape

    def half(lo, hi, K, sh):
        X = np.empty((hi - lo, K), dtype=np.int8)
        for j in range(K):
            kind = (j + sh) % 4
            if kind == 0:
                X[:, j] = q
            elif kind == 1:
                X[:, j] = rng.integers(1, q, size=hi - lo)
            elif kind == 2:
                X[:, j] = rng.integers(1, q + 1, size=hi - lo)
            else:
                X[:, j] = Zo[rng.integers(0, M), lo:hi]
        return np.asfortranarray(X)

    return half(0, split, KA, shift), half(split, N, KB, shift + 1)


def paired_family(N_h, M, held_out, q=21, seed=0x9A12):
    """A paired alignment for the partner-matching check: synth_family at N = 2 N_h draws every sequence -- so both its halves --
    around ONE cluster centre.  -> (Zfit (M, 2 N_h), Zheld (held_out, 2 N_h)): one call generates both, so they share the centres."""
    from gaussdca.jl_amd.synth import synth_family

    Z = synth_family(2 * N_h, M + held_out, q, seed=seed)
    return Z[:M], Z[M:]
