"""Device-resident form of the reference's statement-by-statement pipeline (src/GaussDCA.jl:28-42).

The host-pointer operators of :mod:`dcautils` move every n x n matrix over PCIe twice; a caller who keeps the
reference's six statements should instead keep the arrays in HBM (``DeviceBuffer`` = ``gdca_dbuf``) and call the
``_dev`` entry points of include/gdca.h.  Only ``Z`` goes in and ``S`` comes out.  The functions here carry the
DCAUtils / GaussDCA names with a ``_dev`` suffix and take / return ``DeviceBuffer`` objects (or raw device
pointers as ints, e.g. ``tensor.data_ptr()``); ``gDCA_stepwise`` chains them exactly as ``gDCA`` does at
:28-:42 and gives the same bits as the fused ``gdca_run``.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import _lib
from ._lib import ArgumentError, Context, DeviceBuffer, default_context
from .dcautils import _theta_arg, _zf, compute_ranking


def _ptr(x) -> C.c_void_p:
    return C.c_void_p(x.ptr if isinstance(x, DeviceBuffer) else int(x))


def compute_weights_dev(ctx: Context, dZ, N: int, M: int, theta=":auto", dW=None):
    """compute_weights(Z, q, θ) with Z and W in HBM -> (dW, Meff, theta_used, thresh)"""
    dW = dW or DeviceBuffer(ctx, 8 * M)
    Meff, th, thr = C.c_double(), C.c_double(), C.c_int32()
    ctx.check(ctx.lib.gdca_compute_weights_dev(ctx.h, _ptr(dZ), N, M, _theta_arg(theta), _ptr(dW), C.byref(Meff),
                                               C.byref(th), C.byref(thr)))
    return dW, Meff.value, th.value, int(thr.value)


def compute_weighted_frequencies_dev(ctx: Context, dZ, N: int, M: int, q: int, dW, Meff: float, dPi=None, dPij=None):
    """the accumulation of compute_weighted_frequencies (:28) -> (dPi_true[n], dPij_true[n x n])"""
    n = N * (q - 1)
    dPi = dPi or DeviceBuffer(ctx, 8 * n)
    dPij = dPij or DeviceBuffer(ctx, 8 * n * n)
    ctx.check(ctx.lib.gdca_frequencies_dev(ctx.h, _ptr(dZ), N, M, int(q), _ptr(dW), float(Meff), _ptr(dPi), _ptr(dPij)))
    return dPi, dPij


def add_pseudocount_dev(ctx: Context, dPi_true, dPij_true, N: int, q: int, pc: float, dPi=None, dPij=None):
    """add_pseudocount (:30); in place when no output buffers are given"""
    dPi = dPi or dPi_true
    dPij = dPij or dPij_true
    ctx.check(ctx.lib.gdca_add_pseudocount_dev(ctx.h, _ptr(dPi_true), _ptr(dPij_true), N, int(q), float(pc), _ptr(dPi),
                                               _ptr(dPij)))
    return dPi, dPij


def compute_C_dev(ctx: Context, dPi, dPij, n: int, dC=None):
    """compute_C (:32, :76); C may alias Pij"""
    dC = dC or DeviceBuffer(ctx, 8 * n * n)
    ctx.check(ctx.lib.gdca_covariance_dev(ctx.h, _ptr(dPi), _ptr(dPij), int(n), _ptr(dC)))
    return dC


def inv_cholesky_dev(ctx: Context, dA, n: int):
    """mJ = inv(cholesky(C)) (:34), in place; raises PosDefException(info) like Julia"""
    info = C.c_int32()
    rc = ctx.lib.gdca_spd_inverse_dev(ctx.h, _ptr(dA), int(n), C.byref(info))
    ctx.check(rc, info.value)
    return dA


def inv_cholesky_logdet_dev(ctx: Context, dA, n: int):
    """inv_cholesky_dev and log det C in one call (gdca_spd_inverse_logdet_dev): (dA, logdet), the inverse bit for bit the same"""
    return dA, ctx.spd_inverse_logdet_dev(_ptr(dA).value, int(n))


def compute_FN_dev(ctx: Context, dmJ, N: int, q: int, dS=None):
    dS = dS or DeviceBuffer(ctx, 8 * N * N)
    ctx.check(ctx.lib.gdca_fn_dev(ctx.h, _ptr(dmJ), N, int(q), _ptr(dS)))
    return dS


def compute_DI_gauss_dev(ctx: Context, dmJ, dC, N: int, q: int, dS=None):
    dS = dS or DeviceBuffer(ctx, 8 * N * N)
    ctx.check(ctx.lib.gdca_di_dev(ctx.h, _ptr(dmJ), _ptr(dC), N, int(q), _ptr(dS)))
    return dS


def correct_APC_dev(ctx: Context, dS, N: int):
    ctx.check(ctx.lib.gdca_apc_dev(ctx.h, _ptr(dS), N))
    return dS


def sequence_energies_dev(ctx: Context, dmJ, dPi, N: int, q: int, dX, K: int, dE=None):
    """E[k] = 1/2 (x_k - Pi)' mJ (x_k - Pi) of the K sequences X (N x K int8) with every array in HBM (gdca_energies_dev):
    mJ from inv_cholesky_dev, Pi from add_pseudocount_dev"""
    dE = dE or DeviceBuffer(ctx, 8 * K)
    ctx.energies_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), _ptr(dX).value, int(K), _ptr(dE).value)
    return dE


def pair_energies_dev(ctx: Context, dmJ, dPi, N: int, q: int, split: int, dXA, KA: int, dXB, KB: int, what: int = 1, dE=None):
    """E[a + KA * b] of the KA x KB pairings across the split with every array in HBM (gdca_pair_energies_dev): XA split x KA,
    XB (N - split) x KB int8; what: _lib.PAIR_ENERGY or _lib.PAIR_COUPLING (dPi may then be None)"""
    dE = dE or DeviceBuffer(ctx, 8 * KA * KB)
    ctx.pair_energies_dev(_ptr(dmJ).value, None if dPi is None else _ptr(dPi).value, N, int(q), int(split), _ptr(dXA).value, int(KA),
                          _ptr(dXB).value, int(KB), int(what), _ptr(dE).value)
    return dE


def pair_energies_blocked_dev(ctx: Context, dmJ, dPi, N: int, q: int, split: int, dXA, KA: int, dXB, KB: int, offA, offB, what: int = 1,
                              dE=None):
    """The pairings inside the species of species-sorted sequences with every array in HBM (gdca_pair_energies_blocked_dev): offA /
    offB are HOST offsets (S + 1 each, dcautils.species_blocks); E is packed, block s column-major kA_s x kB_s behind the blocks
    before it (_lib.pair_blocks_length(offA, offB) doubles); every entry bit for bit pair_energies_dev's"""
    dE = dE or DeviceBuffer(ctx, 8 * max(_lib.pair_blocks_length(offA, offB), 1))
    ctx.pair_energies_blocked_dev(_ptr(dmJ).value, None if dPi is None else _ptr(dPi).value, N, int(q), int(split), _ptr(dXA).value, int(KA),
                                  _ptr(dXB).value, int(KB), offA, offB, int(what), _ptr(dE).value)
    return dE


def assign_blocks_dev(ctx: Context, dE, offA, offB, dmatch=None, dgap=None):
    """The minimum-cost assignment inside every block of the packed cost matrix E with every array in HBM (gdca_assign_blocks_dev):
    returns (match int32[KA], gap float64[KA]) as device buffers"""
    KA = int(np.asarray(offA)[-1])
    dmatch = dmatch or DeviceBuffer(ctx, 4 * KA)
    dgap = dgap or DeviceBuffer(ctx, 8 * KA)
    ctx.assign_blocks_dev(_ptr(dE).value, offA, offB, _ptr(dmatch).value, _ptr(dgap).value)
    return dmatch, dgap


def mutation_scan_dev(ctx: Context, dmJ, dPi, N: int, q: int, dX, K: int, what: int = 0, dD=None):
    """D[(b - 1) + q (i + N k)] of every single substitution of the K sequences X (N x K int8) with every array in HBM
    (gdca_mutation_scan_dev): what = _lib.MUT_DELTA (the energy change) or _lib.MUT_POTENTIAL (the site potentials)"""
    dD = dD or DeviceBuffer(ctx, 8 * int(q) * N * K)
    ctx.mutation_scan_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), _ptr(dX).value, int(K), int(what), _ptr(dD).value)
    return dD


def double_mutant_scan_dev(ctx: Context, dmJ, dPi, N: int, q: int, dX, K: int, dEmin=None, dcode=None, depi=None, maps=("Emin", "code", "epi")):
    """The double-mutant maps of the K sequences X (N x K int8) with every array in HBM (gdca_double_mutant_scan_dev): Emin (f64), code
    (int32) and epi (f64), N N K entries each at [i + N (j + N k)].  ``maps`` names the ones wanted; a buffer is made for each of them
    that is not given, the others come back as None.  Returns (dEmin, dcode, depi)."""
    if "Emin" in maps:
        dEmin = dEmin or DeviceBuffer(ctx, 8 * N * N * K)
    if "code" in maps:
        dcode = dcode or DeviceBuffer(ctx, 4 * N * N * K)
    if "epi" in maps:
        depi = depi or DeviceBuffer(ctx, 8 * N * N * K)
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.double_mutant_scan_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), opt(dX), int(K), opt(dEmin), opt(dcode), opt(depi))
    return dEmin, dcode, depi


def double_mutants_dev(ctx: Context, dmJ, dPi, N: int, q: int, dX, K: int, dmuts, L: int, dout=None):
    """ddE of the L listed double mutants (dmuts: 5 x L int32 records (k, i, b, j, c), sites 0-based, symbols 1..q) of the K sequences
    X with every array in HBM (gdca_double_mutants_dev).  Returns dout (L doubles)."""
    dout = dout or DeviceBuffer(ctx, 8 * max(int(L), 1))
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.double_mutants_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), opt(dX), int(K), opt(dmuts), int(L), _ptr(dout).value)
    return dout


def greedy_walk_dev(ctx: Context, dmJ, dPi, N: int, q: int, dX, K: int, max_steps: int, min_gain: float = 0.0, dmask=None, flags: int = 0,
                    dXout=None, dsteps=None, ddE_sum=None, dpath=None, ddE_path=None, dV=None, want=("dE_sum",)):
    """The greedy walk of the K sequences X (N x K int8) to their local energy minima with every array in HBM (gdca_greedy_walk_dev):
    flags = _lib.WALK_GAP_TARGET | _lib.WALK_FILL_GAPS, dmask N int8 or None.  Xout (N x K int8) and steps (K int32) are always
    made; ``want`` names the optional outputs a buffer is made for where none is given: "dE_sum" (K f64), "path" (2 x max_steps x K
    int32), "dE_path" (max_steps x K f64), "V" (q N K f64: the final tables).  Returns (dXout, dsteps, ddE_sum, dpath, ddE_path, dV),
    None for what was not wanted."""
    K, T = int(K), int(max_steps)
    dXout = dXout or DeviceBuffer(ctx, max(N * K, 1))
    dsteps = dsteps or DeviceBuffer(ctx, 4 * max(K, 1))
    if "dE_sum" in want:
        ddE_sum = ddE_sum or DeviceBuffer(ctx, 8 * max(K, 1))
    if "path" in want:
        dpath = dpath or DeviceBuffer(ctx, 8 * max(T * K, 1))
    if "dE_path" in want:
        ddE_path = ddE_path or DeviceBuffer(ctx, 8 * max(T * K, 1))
    if "V" in want:
        dV = dV or DeviceBuffer(ctx, 8 * int(q) * N * max(K, 1))
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.greedy_walk_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), opt(dX), K, opt(dmask), int(flags), float(min_gain), T, opt(dXout),
                        opt(dsteps), opt(ddE_sum), opt(dpath), opt(ddE_path), opt(dV))
    return dXout, dsteps, ddE_sum, dpath, ddE_path, dV


def sample_dev(ctx: Context, dmJ, dPi, N: int, q: int, dX, K: int, beta: float, burn: int, stride: int, n_samples: int, seed: int = 0,
               stream0: int = 0, dmask=None, flags: int = 0, dXs=None, daccepted=None, ddE_s=None, dthr=None, dmoves=None, dV=None,
               want=("dE_s",)):
    """Metropolis chains from the K sequences X (N x K int8) with every array in HBM (gdca_sample_dev): n_steps = burn + n_samples *
    stride proposals a chain, accepted iff beta * dE <= -log(u); flags = _lib.SAMPLE_GAPS or 0, dmask N int8 or None.  Xs (N x n_samples
    x K int8) and accepted (K int32) are always made; ``want`` names the optional outputs a buffer is made for where none is given:
    "dE_s" (n_samples x K f64), "thr" (n_steps x K f64), "moves" (n_steps x K int32), "V" (q N K f64: the final tables).  Returns
    (dXs, daccepted, ddE_s, dthr, dmoves, dV), None for what was not wanted."""
    K, S = int(K), int(n_samples)
    T = int(burn) + S * int(stride)
    dXs = dXs or DeviceBuffer(ctx, max(N * S * K, 1))
    daccepted = daccepted or DeviceBuffer(ctx, 4 * max(K, 1))
    if "dE_s" in want:
        ddE_s = ddE_s or DeviceBuffer(ctx, 8 * max(S * K, 1))
    if "thr" in want:
        dthr = dthr or DeviceBuffer(ctx, 8 * max(T * K, 1))
    if "moves" in want:
        dmoves = dmoves or DeviceBuffer(ctx, 4 * max(T * K, 1))
    if "V" in want:
        dV = dV or DeviceBuffer(ctx, 8 * int(q) * N * max(K, 1))
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.sample_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), opt(dX), K, opt(dmask), int(flags), float(beta), int(seed), int(stream0),
                   int(burn), int(stride), S, opt(dXs), opt(daccepted), opt(ddE_s), opt(dthr), opt(dmoves), opt(dV))
    return dXs, daccepted, ddE_s, dthr, dmoves, dV


def sample_tempered_dev(ctx: Context, dmJ, dPi, N: int, q: int, dXr, K: int, betas, swap_every: int, burn: int, stride: int, n_samples: int,
                        seed: int = 0, stream0: int = 0, dslot0=None, dmask=None, flags: int = 0, dXs=None, daccepted=None, dswaps=None,
                        dXr_out=None, dslot_out=None, dE_s=None, dthr=None, dmoves=None, dswap_thr=None, dslot_path=None, want=("E_s",)):
    """Replica-exchange chains with every array in HBM (gdca_sample_tempered_dev): K chains of R = len(betas) replicas from Xr (N x R x K
    int8; replica r of chain k holds slot dslot0[r + R k], or slot r), each replica a Metropolis chain on stream stream0 + k R + r at
    betas[its slot]; after every swap_every proposals the holders of the slots p, p + 1 (p % 2 == round % 2) exchange slots iff
    (betas[p] - betas[p + 1]) * (E_b - E_a) <= -log(u).  Slot 0 is sampled.  Xs, accepted (R x K, by slot), swaps ((R - 1) x K), Xr_out
    and slot_out are always made; ``want`` names the optional outputs a buffer is made for where none is given: "E_s", "thr", "moves",
    "swap_thr", "slot_path".  Returns (dXs, daccepted, dswaps, dXr_out, dslot_out, dE_s, dthr, dmoves, dswap_thr, dslot_path)."""
    K, S, R = int(K), int(n_samples), len(betas)
    T = int(burn) + S * int(stride)
    E = T // max(int(swap_every), 1)
    G = max(K * R, 1)
    dXs = dXs or DeviceBuffer(ctx, max(N * S * K, 1))
    daccepted = daccepted or DeviceBuffer(ctx, 4 * G)
    dswaps = dswaps or DeviceBuffer(ctx, 4 * max(K * (R - 1), 1))
    dXr_out = dXr_out or DeviceBuffer(ctx, N * G)
    dslot_out = dslot_out or DeviceBuffer(ctx, 4 * G)
    if "E_s" in want:
        dE_s = dE_s or DeviceBuffer(ctx, 8 * max(S * K, 1))
    if "thr" in want:
        dthr = dthr or DeviceBuffer(ctx, 8 * max(T, 1) * G)
    if "moves" in want:
        dmoves = dmoves or DeviceBuffer(ctx, 4 * max(T, 1) * G)
    if "swap_thr" in want:
        dswap_thr = dswap_thr or DeviceBuffer(ctx, 8 * max(E * K * (R - 1), 1))
    if "slot_path" in want:
        dslot_path = dslot_path or DeviceBuffer(ctx, 4 * max(E, 1) * G)
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.sample_tempered_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), opt(dXr), opt(dslot0), K, betas, opt(dmask), int(flags), int(seed),
                            int(stream0), int(swap_every), int(burn), int(stride), S, opt(dXs), opt(daccepted), opt(dswaps), opt(dXr_out),
                            opt(dslot_out), opt(dE_s), opt(dthr), opt(dmoves), opt(dswap_thr), opt(dslot_path))
    return dXs, daccepted, dswaps, dXr_out, dslot_out, dE_s, dthr, dmoves, dswap_thr, dslot_path


def log_partition_dev(ctx: Context, dmJ, dPi, N: int, q: int, betas, sweep: int, K: int, dx=None, dmask=None, flags: int = 0, seed: int = 0,
                      stream0: int = 0, dout=None, dlogw=None, dE_end=None, dX0=None, dXout=None, daccepted=None, dthr=None, dmoves=None,
                      want=()):
    """log Z(betas[-1]) of the Potts reading of (mJ, Pi) by annealed importance sampling with every array in HBM
    (gdca_log_partition_dev): K chains from uniform starts over the state space of the template dx (N int8; None: every site is free,
    and then no mask), L = len(betas) - 1 stages of ``sweep`` proposals, betas[0] == 0.  out4 (log Z, effective sample size, max logw,
    log |Omega|) and logw (K f64) are always made; ``want`` names the optional outputs a buffer is made for where none is given: "E_end"
    (K f64), "X0", "Xout" (N x K int8), "accepted" (K int32), "thr" (n_steps x K f64), "moves" (n_steps x K int32).  Returns (dout,
    dlogw, dE_end, dX0, dXout, daccepted, dthr, dmoves), None for what was not wanted."""
    K, T = int(K), (len(betas) - 1) * int(sweep)
    dout = dout or DeviceBuffer(ctx, 32)
    dlogw = dlogw or DeviceBuffer(ctx, 8 * max(K, 1))
    if "E_end" in want:
        dE_end = dE_end or DeviceBuffer(ctx, 8 * max(K, 1))
    if "X0" in want:
        dX0 = dX0 or DeviceBuffer(ctx, max(N * K, 1))
    if "Xout" in want:
        dXout = dXout or DeviceBuffer(ctx, max(N * K, 1))
    if "accepted" in want:
        daccepted = daccepted or DeviceBuffer(ctx, 4 * max(K, 1))
    if "thr" in want:
        dthr = dthr or DeviceBuffer(ctx, 8 * max(T * K, 1))
    if "moves" in want:
        dmoves = dmoves or DeviceBuffer(ctx, 4 * max(T * K, 1))
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.log_partition_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), opt(dx), opt(dmask), int(flags), betas, int(sweep), K, int(seed),
                          int(stream0), opt(dout), opt(dlogw), opt(dE_end), opt(dX0), opt(dXout), opt(daccepted), opt(dthr), opt(dmoves))
    return dout, dlogw, dE_end, dX0, dXout, daccepted, dthr, dmoves


def potts_from_gaussian_dev(ctx: Context, dmJ, dPi, N: int, q: int, dW=None):
    """The Gaussian model (mJ, Pi) as a Potts model (W, zeros) in mJ's layout, every array in HBM (gdca_potts_from_gaussian_dev):
    off-diagonal blocks the bits of mJ, W[r, r] = mJ[r, r] - 2 (mJ Pi)[r], the rest of a diagonal block +0.0.  W may not be mJ."""
    n = N * (int(q) - 1)
    dW = dW or DeviceBuffer(ctx, 8 * n * n)
    ctx.potts_from_gaussian_dev(_ptr(dmJ).value, _ptr(dPi).value, N, int(q), _ptr(dW).value)
    return dW


def bm_update_dev(ctx: Context, dW, dPij_d, dPij_m, N: int, q: int, eta: float, lam: float = 0.0, dPi_d=None, dPi_m=None):
    """One Boltzmann-machine step on W in place (gdca_bm_update_dev): W += eta (m (Pij_m - Pij_d) - [m == 1] lam W), m = 2 on the
    diagonal, 0 elsewhere inside a diagonal block, 1 outside.  The single-site tallies are not read."""
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.bm_update_dev(_ptr(dW).value, _ptr(dPij_d).value, _ptr(dPij_m).value, N, int(q), float(eta), float(lam), opt(dPi_d), opt(dPi_m))
    return dW


def bm_readout_dev(ctx: Context, dPi_d, dPij_d, dPi_m, dPij_m, N: int, q: int, dout=None):
    """The fit of the model's tallies to the data's (gdca_bm_readout_dev) -> a buffer of four f64: max |Pi_m - Pi_d|, max |c_m - c_d|
    and the Pearson correlation of c_m and c_d over the off-diagonal blocks (c = Pij - Pi Pi'), then +0.0."""
    dout = dout or DeviceBuffer(ctx, 32)
    ctx.bm_readout_dev(_ptr(dPi_d).value, _ptr(dPij_d).value, _ptr(dPi_m).value, _ptr(dPij_m).value, N, int(q), _ptr(dout).value)
    return dout


def bm_learn_dev(ctx: Context, dW, dPi_d, dPij_d, N: int, q: int, dX, K: int, n_iter: int, burn: int, stride: int, n_samples: int,
                 eta: float, lam: float = 0.0, beta: float = 1.0, seed: int = 0, iter0: int = 0, dmask=None, flags: int = 0, dtrace=None,
                 dXs_last=None):
    """n_iter iterations of Boltzmann-machine learning with every array in HBM and no host round trip per iteration
    (gdca_bm_learn_dev): sample K persistent chains under (W, zeros) from X (N x K int8), tally the K n_samples samples, read the
    fit out into trace[4 i ..], update W.  W and X change in place; a later call continues with ``iter0 + n_iter``.  Returns dtrace
    (4 x n_iter f64: max |dPi|, max |dc|, Pearson, acceptance rate per iteration)."""
    dtrace = dtrace or DeviceBuffer(ctx, 32 * max(int(n_iter), 1))
    opt = lambda b: None if b is None else _ptr(b).value  # noqa: E731
    ctx.bm_learn_dev(_ptr(dW).value, _ptr(dPi_d).value, _ptr(dPij_d).value, N, int(q), opt(dX), int(K), opt(dmask), int(flags), float(beta),
                     int(seed), int(iter0), int(n_iter), int(burn), int(stride), int(n_samples), float(eta), float(lam), _ptr(dtrace).value,
                     opt(dXs_last))
    return dtrace


def bm_learn_tempered_dev(ctx: Context, dW, dPi_d, dPij_d, N: int, q: int, dXr, dslot, K: int, betas, n_iter: int, burn: int, stride: int,
                          n_samples: int, eta: float, lam: float = 0.0, swap_every=None, seed: int = 0, iter0: int = 0, dmask=None,
                          flags: int = 0):
    """n_iter iterations of Boltzmann-machine learning with REPLICA-EXCHANGE chains, driven from the host over the operator forms with
    every array in HBM: iteration t runs sample_tempered_dev under (W, zeros) with stream0 = t K R from the persistent replicas dXr
    (N x R x K int8) and their slots dslot (R x K int32, or None: replica r holds slot r), keeps Xr_out / slot_out as the next
    iteration's start, tallies the K n_samples samples of slot 0 (betas[0], the target temperature), reads the fit out and updates W in
    place.  One download of R K counts an iteration is the loop's only host round trip.  With betas = (beta,) the model, the chains
    and the trace are bm_learn_dev's bit for bit.  Returns (dXr, dslot, trace (n_iter, 4), swap_rates (n_iter, R - 1)): the final
    replicas and slots (new buffers), trace as bm_learn_dev's with the acceptance rate of slot 0 in column 3, and the accepted
    fraction of every pair's attempted swaps per iteration."""
    K, S, R, n_iter = int(K), int(n_samples), len(betas), int(n_iter)
    n, T, M = N * (int(q) - 1), int(burn) + S * int(stride), K * S
    every = N if swap_every is None else int(swap_every)
    E = T // max(every, 1)
    att = np.array([(E - p % 2 + 1) // 2 for p in range(R - 1)], dtype=np.float64)  # the rounds e < E with e % 2 == p % 2
    dZero, dOnes = DeviceBuffer.from_array(ctx, np.zeros(n)), DeviceBuffer.from_array(ctx, np.ones(M))
    dPi_m, dPij_m, dout = DeviceBuffer(ctx, 8 * n), DeviceBuffer(ctx, 8 * n * n), DeviceBuffer(ctx, 32)
    G = K * R
    pairs = [(DeviceBuffer(ctx, N * G), DeviceBuffer(ctx, 4 * G)) for _ in range(2)]  # (Xr_out may alias nothing that is read)
    src = (dXr, dslot)
    dXs, dacc, dsw = DeviceBuffer(ctx, max(N * M, 1)), DeviceBuffer(ctx, 4 * G), DeviceBuffer(ctx, 4 * max(K * (R - 1), 1))
    trace, rates = np.empty((n_iter, 4)), np.empty((n_iter, R - 1))
    for it in range(n_iter):
        t = int(iter0) + it
        dst = pairs[it % 2]
        sample_tempered_dev(ctx, dW, dZero, N, q, src[0], K, betas, every, burn, stride, S, seed, t * G, dslot0=src[1], dmask=dmask,
                            flags=flags, dXs=dXs, daccepted=dacc, dswaps=dsw, dXr_out=dst[0], dslot_out=dst[1], want=())
        src = dst  # (the caller's buffers are never written)
        compute_weighted_frequencies_dev(ctx, dXs, N, M, q, dOnes, float(M), dPi_m, dPij_m)
        bm_readout_dev(ctx, dPi_d, dPij_d, dPi_m, dPij_m, N, q, dout)
        trace[it] = dout.download((4,))
        acc = dacc.download((K, R), np.int32, order="C")
        trace[it, 3] = np.float64(int(acc[:, 0].astype(np.int64).sum())) / np.float64(K * T)
        if R > 1:
            rates[it] = dsw.download((K, R - 1), np.int32, order="C").astype(np.int64).sum(axis=0) / (K * att)
        bm_update_dev(ctx, dW, dPij_d, dPij_m, N, q, eta, lam)
    for b in (dZero, dOnes, dPi_m, dPij_m, dout, dXs, dacc, dsw) + pairs[n_iter % 2]:
        b.free()
    return src[0], src[1], trace, rates


def bm_fit(Z, q: int, n_iter: int, K: int = 1024, eta: float = 1.0, lam: float = 0.0, pseudocount: float = 0.8,
           target_pseudocount: float = 0.0, theta=":auto", init: str = "gaussian", burn=None, stride=None, n_samples: int = 1,
           beta: float = 1.0, seed: int = 0, gaps: bool = True, scores: bool = False, ctx: Context = None, betas=None, swap_every=None,
           plm_iter: int = 100, plm_lam: float = 0.01):
    """Boltzmann-machine refinement built like scores_stepwise from the device operators.  Z: (N, M) int8.  weights, frequencies,
    pseudocount, covariance, inverse (the warm start, ``init="gaussian"``; "independent" skips the last two; "plm": the
    independent-site model moved by ``plm_iter`` pseudo-likelihood iterations, plm_learn_dev at its default step with the penalty
    ``plm_lam``, towards the same target frequencies), then n_iter iterations
    of bm_learn_dev towards the frequencies at ``target_pseudocount``.  The chains start from the first K sequences of Z (K <= M).
    Returns (W (n, n), trace (n_iter, 4)) and, with ``scores=True``, S = APC(FN(W)) as a third entry.
    ``betas`` (a ladder, the target temperature first; ``beta`` is then not used): the iterations are bm_learn_tempered_dev's, every
    replica of chain k starting at sequence k, swaps every ``swap_every`` proposals (default N); the swap rates (n_iter, R - 1) come
    back as a third entry, before S."""
    from .dcautils import potts_independent

    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    if init not in ("gaussian", "independent", "plm"):
        raise ArgumentError(f"invalid init value: {init} (must be \"gaussian\", \"independent\" or \"plm\")")
    if init == "plm" and (not isinstance(plm_iter, (int, np.integer)) or plm_iter < 1):
        raise ArgumentError(f"invalid plm_iter value: {plm_iter} (must be an integer >= 1)")
    if not isinstance(K, (int, np.integer)) or not 1 <= K <= M:
        raise ArgumentError(f"invalid K value: {K} (must be an integer between 1 and the number of sequences, {M})")
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ArgumentError(f"invalid n_iter value: {n_iter} (must be an integer >= 1)")
    n = N * (q - 1)
    burn = 10 * N if burn is None else int(burn)
    stride = N if stride is None else int(stride)
    dZ = DeviceBuffer.from_array(ctx, Zf)
    dW_, Meff, th, thr = compute_weights_dev(ctx, dZ, N, M, theta)
    dPi_t, dPij_t = compute_weighted_frequencies_dev(ctx, dZ, N, M, q, dW_, Meff)
    # the target: the family's frequencies at target_pseudocount
    dPi_d, dPij_d = add_pseudocount_dev(ctx, dPi_t, dPij_t, N, q, target_pseudocount, DeviceBuffer(ctx, 8 * n), DeviceBuffer(ctx, 8 * n * n))
    # the start
    dPi, dPij = add_pseudocount_dev(ctx, dPi_t, dPij_t, N, q, pseudocount)
    if init == "gaussian":
        dmJ = compute_C_dev(ctx, dPi, dPij, n, dC=dPij)
        inv_cholesky_dev(ctx, dmJ, n)
        dW = potts_from_gaussian_dev(ctx, dmJ, dPi, N, q)
    else:
        dW = DeviceBuffer.from_array(ctx, potts_independent(dPi.download((n,)), N, q))
        if init == "plm":
            plm_learn_dev(ctx, dW, dZ, dW_, Meff, dPi_d, dPij_d, N, M, q, int(plm_iter), 1.0 / (N + 2.0 * float(plm_lam)),
                          float(plm_lam)).free()
    dX = DeviceBuffer.from_array(ctx, np.asfortranarray(Zf[:, :K]))
    if betas is None:
        dtrace = bm_learn_dev(ctx, dW, dPi_d, dPij_d, N, q, dX, K, n_iter, burn, stride, n_samples, eta, lam, beta, seed,
                              flags=_lib.SAMPLE_GAPS if gaps else 0)
        W, trace = dW.download((n, n)), dtrace.download((int(n_iter), 4), order="C")
        out = (W, trace)
    else:
        R = len(betas)
        dXr0 = DeviceBuffer.from_array(ctx, np.asfortranarray(np.repeat(Zf[:, None, :K], R, axis=1)))  # (N, R, K): the replicas' starts
        dXr, dslot, trace, rates = bm_learn_tempered_dev(ctx, dW, dPi_d, dPij_d, N, q, dXr0, None, K, betas, n_iter, burn, stride, n_samples,
                                                         eta, lam, swap_every, seed, flags=_lib.SAMPLE_GAPS if gaps else 0)
        dtrace = dXr0  # (freed with the rest below)
        dXr.free(), dslot.free()
        out = (dW.download((n, n)), trace, rates)
    if scores:
        dS = correct_APC_dev(ctx, compute_FN_dev(ctx, dW, N, q), N)
        out += (dS.download((N, N)),)
        dS.free()
    for b in (dZ, dW_, dPi_t, dPij_t, dPi_d, dPij_d, dW, dX, dtrace):
        b.free()
    return out


def plm_conditionals_dev(ctx: Context, dW, dZ, N: int, M: int, q: int, dp=None, dnll_k=None):
    """The conditionals of the M sequences Z (N x M int8) under the Potts model (W, zeros), every array in HBM
    (gdca_plm_conditionals_dev) -> (dp, dnll_k): p[(c - 1) + q (i + N k)] = P(x_i = c | the rest of sequence k) (the scan's layout,
    the gap last; q N M f64) and nll_k[k] = -sum_i log P(x_ki | rest)."""
    dp = dp or DeviceBuffer(ctx, 8 * int(q) * N * M)
    dnll_k = dnll_k or DeviceBuffer(ctx, 8 * M)
    ctx.plm_conditionals_dev(_ptr(dW).value, _ptr(dZ).value, N, M, int(q), _ptr(dp).value, _ptr(dnll_k).value)
    return dp, dnll_k


def plm_tally_dev(ctx: Context, dp, dZ, dw, Meff: float, N: int, M: int, q: int, dPi_c=None, dPij_c=None):
    """The conditional tallies (gdca_plm_tally_dev) of the conditionals p against Z with the weights w -> (dPi_c[n], dPij_c[n x n]),
    in the frequencies' layout; summed in the fixed order include/gdca.h states (context option PLM_CHUNK)."""
    n = N * (int(q) - 1)
    dPi_c = dPi_c or DeviceBuffer(ctx, 8 * n)
    dPij_c = dPij_c or DeviceBuffer(ctx, 8 * n * n)
    ctx.plm_tally_dev(_ptr(dp).value, _ptr(dZ).value, _ptr(dw).value, float(Meff), N, M, int(q), _ptr(dPi_c).value, _ptr(dPij_c).value)
    return dPi_c, dPij_c


def plm_tallies_dev(ctx: Context, dW, dZ, dw, Meff: float, N: int, M: int, q: int, dPi_c=None, dPij_c=None, dnll=None):
    """plm_conditionals_dev and plm_tally_dev fused over slabs of sequences (gdca_plm_tallies_dev; the same bits) ->
    (dPi_c, dPij_c, dnll): dnll holds one f64, nll = (sum_k w_k nll_k) / Meff.  2 (Pij_c - Pij_d) is the gradient of the log
    pseudo-likelihood by the couplings, 1/2 (Pi_c - Pi_d) by W's diagonal."""
    n = N * (int(q) - 1)
    dPi_c = dPi_c or DeviceBuffer(ctx, 8 * n)
    dPij_c = dPij_c or DeviceBuffer(ctx, 8 * n * n)
    dnll = dnll or DeviceBuffer(ctx, 8)
    ctx.plm_tallies_dev(_ptr(dW).value, _ptr(dZ).value, _ptr(dw).value, float(Meff), N, M, int(q), _ptr(dPi_c).value, _ptr(dPij_c).value,
                        _ptr(dnll).value)
    return dPi_c, dPij_c, dnll


def plm_learn_dev(ctx: Context, dW, dZ, dw, Meff: float, dPi_d, dPij_d, N: int, M: int, q: int, n_iter: int, eta: float, lam: float = 0.0,
                  dtrace=None):
    """n_iter iterations of pseudo-likelihood ascent on W in place with every array in HBM and no host round trip per iteration
    (gdca_plm_learn_dev): tallies, read-out, bm_update_dev's step.  Returns dtrace (4 x n_iter f64: max |Pi_c - Pi_d|, max |dc|,
    Pearson, nll per iteration, each of the W the iteration started from).  A later call continues the same run bit for bit."""
    dtrace = dtrace or DeviceBuffer(ctx, 32 * max(int(n_iter), 1))
    ctx.plm_learn_dev(_ptr(dW).value, _ptr(dZ).value, _ptr(dw).value, float(Meff), _ptr(dPi_d).value, _ptr(dPij_d).value, N, M, int(q),
                      int(n_iter), float(eta), float(lam), _ptr(dtrace).value)
    return dtrace


PLM_GROW = 1.2  # the factor of plm_learn_adaptive_dev


def plm_penalty(W, N: int, q: int) -> float:
    """sum_{i<j} |W_ij|^2 of the couplings of W (n, n): the squares of the entries below the diagonal blocks, summed by numpy's
    ``sum`` of the masked square (what the adaptive rule compares; tests/plm_model.py takes the same sum)."""
    s = int(q) - 1
    site = np.arange(N * s) // s
    return float(np.sum(np.where(site[:, None] > site[None, :], np.asarray(W) ** 2, 0.0)))


def plm_learn_adaptive_dev(ctx: Context, dW, dZ, dw, Meff: float, dPi_d, dPij_d, N: int, M: int, q: int, n_iter: int, eta: float,
                           lam: float = 0.0, state=None):
    """Pseudo-likelihood ascent with an adapted step, driven from the host over the operator forms (bm_learn_tempered_dev's pattern;
    one download of W and of five f64 an iteration).  THE RULE, deterministic: every iteration evaluates the tallies and
    f = nll + lam * plm_penalty(W) at the current W.  If there is no accepted point yet, or f < f_acc: the point is ACCEPTED -- eta
    grows by PLM_GROW (not at the first point), f_acc = f, W is kept in a device copy --; f == f_acc: accepted, eta stays; then the
    step bm_update_dev(eta).  If f > f_acc (a rise; a NaN counts as one): W is restored from the copy, eta is halved, nothing else --
    the next iteration evaluates the restored point again.  So a step size is never kept after a rise.
    Returns (trace (n_iter, 4) as plm_learn_dev's, etas (n_iter,): the eta each iteration stepped with, 0.0 where it restored,
    state): ``state`` (eta, f_acc, the device copy) passed to a later call continues the run to the same bits."""
    n = N * (int(q) - 1)
    n_iter = int(n_iter)
    eta, f_acc, dsave = (float(eta), None, DeviceBuffer(ctx, 8 * n * n)) if state is None else (state["eta"], state["f_acc"], state["dsave"])
    dPi_c, dPij_c, dnll, dout = DeviceBuffer(ctx, 8 * n), DeviceBuffer(ctx, 8 * n * n), DeviceBuffer(ctx, 8), DeviceBuffer(ctx, 32)
    trace, etas = np.empty((n_iter, 4)), np.zeros(n_iter)
    for it in range(n_iter):
        plm_tallies_dev(ctx, dW, dZ, dw, Meff, N, M, q, dPi_c, dPij_c, dnll)
        bm_readout_dev(ctx, dPi_d, dPij_d, dPi_c, dPij_c, N, q, dout)
        trace[it] = dout.download((4,))
        nll = float(dnll.download((1,))[0])
        trace[it, 3] = nll
        f = nll + float(lam) * plm_penalty(dW.download((n, n)), N, q) if lam else nll
        if f_acc is None or f <= f_acc:
            if f_acc is not None and f < f_acc:
                eta *= PLM_GROW
            f_acc = f
            dsave.copy_from(dW, 8 * n * n)
            bm_update_dev(ctx, dW, dPij_d, dPij_c, N, q, eta, lam)
            etas[it] = eta
        else:
            dW.copy_from(dsave, 8 * n * n)
            eta *= 0.5
    for b in (dPi_c, dPij_c, dnll, dout):
        b.free()
    return trace, etas, {"eta": eta, "f_acc": f_acc, "dsave": dsave}


def plm_fit(Z, q: int, n_iter: int, lam: float = 0.01, eta=None, init: str = "independent", adapt: bool = False, pseudocount: float = 0.8,
            target_pseudocount: float = 0.0, theta=":auto", scores: bool = False, ctx: Context = None):
    """The pseudo-likelihood fit built like bm_fit from the device operators.  Z: (N, M) int8.  weights, frequencies, the start
    (``init="independent"``: the independent-site model of the frequencies at ``pseudocount``; "gaussian": pseudocount, covariance,
    inverse, potts_from_gaussian_dev), then n_iter iterations of plm_learn_dev -- ``adapt=True``: of plm_learn_adaptive_dev -- with the
    family's frequencies at ``target_pseudocount`` as the data's side of the gradient.  ``eta=None`` is 1 / (N + 2 lam).
    Returns (W (n, n), trace (n_iter, 4)) and, with ``scores=True``, S = APC(FN(W)) as a third entry."""
    from .dcautils import potts_independent

    Zf = _zf(Z)
    N, M = Zf.shape
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    if init not in ("gaussian", "independent"):
        raise ArgumentError(f"invalid init value: {init} (must be \"gaussian\" or \"independent\")")
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ArgumentError(f"invalid n_iter value: {n_iter} (must be an integer >= 1)")
    if not isinstance(lam, (int, float, np.integer, np.floating)) or not np.isfinite(lam) or lam < 0:
        raise ArgumentError(f"invalid lam value: {lam}")
    eta = 1.0 / (N + 2.0 * float(lam)) if eta is None else eta
    if not isinstance(eta, (int, float, np.integer, np.floating)) or not np.isfinite(eta) or eta <= 0:
        raise ArgumentError(f"invalid eta value: {eta}")
    ctx = ctx or default_context()
    n = N * (q - 1)
    dZ = DeviceBuffer.from_array(ctx, Zf)
    dw, Meff, th, thr = compute_weights_dev(ctx, dZ, N, M, theta)
    dPi_t, dPij_t = compute_weighted_frequencies_dev(ctx, dZ, N, M, q, dw, Meff)
    dPi_d, dPij_d = add_pseudocount_dev(ctx, dPi_t, dPij_t, N, q, target_pseudocount, DeviceBuffer(ctx, 8 * n), DeviceBuffer(ctx, 8 * n * n))
    dPi, dPij = add_pseudocount_dev(ctx, dPi_t, dPij_t, N, q, pseudocount)
    if init == "gaussian":
        dmJ = compute_C_dev(ctx, dPi, dPij, n, dC=dPij)
        inv_cholesky_dev(ctx, dmJ, n)
        dW = potts_from_gaussian_dev(ctx, dmJ, dPi, N, q)
    else:
        dW = DeviceBuffer.from_array(ctx, potts_independent(dPi.download((n,)), N, q))
    if adapt:
        trace, _, state = plm_learn_adaptive_dev(ctx, dW, dZ, dw, Meff, dPi_d, dPij_d, N, M, q, n_iter, float(eta), float(lam))
        state["dsave"].free()
    else:
        dtrace = plm_learn_dev(ctx, dW, dZ, dw, Meff, dPi_d, dPij_d, N, M, q, n_iter, float(eta), float(lam))
        trace = dtrace.download((int(n_iter), 4), order="C")
        dtrace.free()
    out = (dW.download((n, n)), trace)
    if scores:
        dS = correct_APC_dev(ctx, compute_FN_dev(ctx, dW, N, q), N)
        out += (dS.download((N, N)),)
        dS.free()
    for b in (dZ, dw, dPi_t, dPij_t, dPi_d, dPij_d, dW):
        b.free()
    return out


def scores_stepwise(Z, q: int, pseudocount: float = 0.8, theta=":auto", score: str = "frob", ctx: Context = None
                    ) -> Tuple[np.ndarray, dict]:
    """The six statements of src/GaussDCA.jl:28-42 one by one, arrays resident in HBM.  Z: (N, M) int8.
    Returns (S[N, N], dict(theta, thresh, Meff))."""
    ctx = ctx or default_context()
    Zf = _zf(Z)
    N, M = Zf.shape
    if q >= 32:
        raise ArgumentError(f"parameter q={q} is too big (max 31 is allowed)")
    n = N * (q - 1)
    dZ = DeviceBuffer.from_array(ctx, Zf)
    # Pi_true, Pij_true, Meff, _ = compute_weighted_frequencies(Z, q, θ)                      (:28)
    dW, Meff, th, thr = compute_weights_dev(ctx, dZ, N, M, theta)
    dPi, dPij = compute_weighted_frequencies_dev(ctx, dZ, N, M, q, dW, Meff)
    # Pi, Pij = add_pseudocount(Pi_true, Pij_true, Float64(pseudocount), q)                   (:30)
    add_pseudocount_dev(ctx, dPi, dPij, N, q, pseudocount)
    # C = compute_C(Pi, Pij)                                                                  (:32)
    is_di = str(score).lstrip(":") == "DI"
    dC = compute_C_dev(ctx, dPi, dPij, n) if is_di else None      # compute_DI_gauss needs C as well as mJ
    dmJ = compute_C_dev(ctx, dPi, dPij, n, dC=dPij)
    # mJ = inv(cholesky(C))                                                                   (:34)
    inv_cholesky_dev(ctx, dmJ, n)
    # S = compute_DI_gauss(mJ, C, q) | compute_FN(mJ, q)                                      (:36-40)
    dS = compute_DI_gauss_dev(ctx, dmJ, dC, N, q) if is_di else compute_FN_dev(ctx, dmJ, N, q)
    # S = correct_APC(S)                                                                      (:42)
    correct_APC_dev(ctx, dS, N)
    S = dS.download((N, N))
    for b in (dZ, dW, dPi, dPij, dS) + ((dC,) if dC is not None else ()):
        b.free()
    return S, dict(theta=th, thresh=thr, Meff=Meff)


def gDCA_stepwise(Z, q: int, pseudocount: float = 0.8, theta=":auto", score: str = "frob", min_separation: int = 5,
                  ctx: Context = None):
    S, _ = scores_stepwise(Z, q, pseudocount, theta, score, ctx)
    return compute_ranking(S, int(min_separation))
