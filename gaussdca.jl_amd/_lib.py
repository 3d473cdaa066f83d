"""ctypes binding of libgdca.so (include/gdca.h).  There is no CPU fallback: if the shared
library is missing or no HIP device is usable, every entry point raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GDCA_LIB: another build of the same library (kernel experiments: tools/exp_*.sh build variants beside the product)
LIB_PATH = os.environ.get("GDCA_LIB") or os.path.join(_HERE, "libgdca.so")

GDCA_OK, GDCA_EINVAL, GDCA_ENOTPD, GDCA_EHIP, GDCA_ENOMEM, GDCA_ENOCONV = 0, 1, 2, 3, 4, 5
SCORE_FROB, SCORE_DI = 0, 1
PAIR_COUPLING, PAIR_ENERGY = 0, 1  # `what` of gdca_pair_energies: the cross-term matrix R alone, or the energy of every concatenation
MUT_DELTA, MUT_POTENTIAL = 0, 1  # `what` of gdca_mutation_scan: the energy change of every substitution, or the site potentials themselves
WALK_GAP_TARGET, WALK_FILL_GAPS = 1, 2  # `flags` of gdca_greedy_walk: the gap is a target ("delete"); a gap site may receive a residue
WALK_MAX_STEPS = 65535  # GDCA_WALK_MAX_STEPS
_NO_SWAPS = np.zeros(1, dtype=np.int32)  # what `swaps` points at where a chain has one replica (never written)
TEMPER_MAX = 64  # GDCA_TEMPER_MAX: the most replicas a chain of gdca_sample_tempered may have
SAMPLE_GAPS = 1  # `flags` of gdca_sample: the gap is a symbol like any other (default: residues change into residues, gaps stay gaps)
ABI_VERSION = 6  # GDCA_VERSION_MAJOR * 1000 + GDCA_VERSION_MINOR of the header this binding mirrors


class GdcaError(RuntimeError):
    pass


class ArgumentError(ValueError):
    """Mirror of Julia's ArgumentError thrown by check_arguments (src/GaussDCA.jl:49-65)."""


class PosDefException(ArithmeticError):
    """Mirror of LinearAlgebra.PosDefException(info) thrown by cholesky (src/GaussDCA.jl:34)."""

    def __init__(self, info: int):
        super().__init__(f"matrix is not positive definite; Cholesky factorization failed (info={info})")
        self.info = int(info)


class ConvergenceError(ArithmeticError):
    """Mirror of the LAPACKException an eigenvalue routine raises inside DCAUtils.compute_DI_gauss
    (src/GaussDCA.jl:37) when its iteration does not converge."""

    def __init__(self, npairs: int):
        super().__init__(f"eigenvalue iteration did not converge for {npairs} site pair(s)")
        self.npairs = int(npairs)


class Params(C.Structure):
    _fields_ = [("pseudocount", C.c_double), ("theta", C.c_double), ("score", C.c_int32), ("apc", C.c_int32)]


# the columns of a row of gdca_run_partner_ipa's rounds_out (GDCA_IPA_*), GDCA_IPA_FIELDS of them
IPA_FIELDS = ("M_train", "candidates", "n_sel", "n_changed", "Meff", "theta", "logdet", "cost", "ms_fit", "ms_match", "ms_select", "reserved")

# the entries of gdca_run_pair_logodds' / gdca_run_partner_logodds' info (GDCA_LOGODDS_*), GDCA_LOGODDS_FIELDS of them
LOGODDS_FIELDS = ("logdet", "logdet_A", "logdet_B", "information", "refined_A", "refined_B", "ms_marginals", "reserved")

MULTI_MAX = 16  # GDCA_MULTI_MAX: settings one gdca_run_multi call takes


def _multi_params(settings, theta: float, apc: bool):
    """settings: (pseudocount, score) or (pseudocount, score, apc) per member, score SCORE_FROB | SCORE_DI -> a Params[K] array"""
    K = len(settings)
    prm = (Params * max(K, 1))()
    for k, s in enumerate(settings):
        pc, score = s[0], s[1]
        a = s[2] if len(s) > 2 else apc
        prm[k] = Params(float(pc), float(theta), int(score), 1 if a else 0)
    return prm, K


class Stats(C.Structure):
    _fields_ = [
        ("theta", C.c_double), ("Meff", C.c_double), ("pair_identity_sum", C.c_uint64),
        ("thresh", C.c_int32), ("info", C.c_int32),
        ("N", C.c_int32), ("M", C.c_int32), ("q", C.c_int32), ("n", C.c_int32), ("n_pad", C.c_int32),
        ("update_launches", C.c_int32), ("inverse_batch", C.c_int32), ("refined", C.c_int32),
        ("ms_total", C.c_double), ("ms_theta", C.c_double), ("ms_weights", C.c_double),
        ("ms_covariance", C.c_double), ("ms_inverse", C.c_double), ("ms_inverse_update", C.c_double),
        ("ms_score", C.c_double), ("inverse_flops", C.c_double), ("update_flops", C.c_double),
        ("sweep_ghz", C.c_double), ("inverse_norm1", C.c_double), ("matrix_norm1", C.c_double), ("cond_bound", C.c_double),
        ("ms_fn", C.c_double), ("ms_pair_tally", C.c_double), ("sweep_retries", C.c_int32), ("reserved0", C.c_int32),   # (new fields go to the END: an older build of the library fills a prefix)
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/gdca.h declares: name -> (restype, argtypes)
_i8p, _i32p, _f64p, _u64p = C.POINTER(C.c_int8), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
_ctx = C.c_void_p
SYMBOLS = {
    "gdca_version": (C.c_int32, []),
    "gdca_stats_bytes": (C.c_int32, []),
    "gdca_params_bytes": (C.c_int32, []),
    "gdca_device_count": (C.c_int32, []),
    "gdca_ctx_create": (C.c_int, [C.c_int32, C.POINTER(_ctx)]),
    "gdca_ctx_create_on_stream": (C.c_int, [C.c_int32, C.c_void_p, C.POINTER(_ctx)]),
    "gdca_ctx_create_peer": (C.c_int, [_ctx, C.POINTER(_ctx)]),
    "gdca_ctx_destroy": (C.c_int, [_ctx]),
    "gdca_ctx_synchronize": (C.c_int, [_ctx]),
    "gdca_last_error": (C.c_char_p, [_ctx]),
    "gdca_ctx_set_timing": (C.c_int, [_ctx, C.c_int32]),
    "gdca_ctx_set_option": (C.c_int, [_ctx, C.c_char_p, C.c_char_p]),
    "gdca_run": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p,
                           C.POINTER(Stats)]),
    "gdca_run_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p,
                               C.POINTER(Stats)]),
    "gdca_run_dev_async": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p]),
    "gdca_run_collect": (C.c_int, [_ctx, C.POINTER(Stats)]),
    "gdca_run_dev_phased": (C.c_int, [C.POINTER(_ctx), C.c_int32, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.POINTER(Params),
                                      C.POINTER(C.c_void_p)]),
    "gdca_dbuf_alloc": (C.c_int, [_ctx, C.c_uint64, C.POINTER(C.c_void_p)]),
    "gdca_dbuf_free": (C.c_int, [C.c_void_p]),
    "gdca_dbuf_ptr": (C.c_void_p, [C.c_void_p]),
    "gdca_dbuf_bytes": (C.c_uint64, [C.c_void_p]),
    "gdca_dbuf_upload": (C.c_int, [_ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "gdca_dbuf_download": (C.c_int, [_ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "gdca_dbuf_copy": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_uint64]),
    "gdca_pair_identity_sum_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, _u64p]),
    "gdca_compute_theta_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, _f64p]),
    "gdca_neighbour_counts_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_compute_weights_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, _f64p,
                                           _f64p, _i32p]),
    "gdca_frequencies_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double,
                                       C.c_void_p, C.c_void_p]),
    "gdca_add_pseudocount_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                           C.c_void_p]),
    "gdca_covariance_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gdca_spd_inverse_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _i32p]),
    "gdca_spd_inverse_batch_dev": (C.c_int, [C.POINTER(_ctx), C.c_int32, C.POINTER(C.c_void_p), _i32p, _i32p]),
    "gdca_fn_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_di_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_apc_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32]),
    "gdca_pair_identity_sum": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, _u64p]),
    "gdca_compute_theta": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, _f64p]),
    "gdca_neighbour_counts": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_compute_weights": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, _f64p, _f64p,
                                       _i32p]),
    "gdca_frequencies": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double,
                                   C.c_void_p, C.c_void_p]),
    "gdca_add_pseudocount": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                       C.c_void_p]),
    "gdca_covariance": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gdca_spd_inverse": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _i32p]),
    "gdca_fn": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_di": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_apc": (C.c_int, [_ctx, C.c_void_p, C.c_int32]),
    "gdca_host_cpus": (C.c_int32, []),
    "gdca_fasta_open": (C.c_int, [C.c_char_p, C.c_double, C.POINTER(C.c_void_p), _i32p, _i32p]),
    "gdca_fasta_copy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gdca_fasta_data": (C.c_void_p, [C.c_void_p]),
    "gdca_fasta_max_symbol": (C.c_int32, [C.c_void_p]),
    "gdca_fasta_close": (C.c_int, [C.c_void_p]),
    "gdca_remove_duplicates": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, _i32p]),
    "gdca_ranking_length": (C.c_int64, [C.c_int32, C.c_int32]),
    "gdca_ranking": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_ranking_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_run_ranked_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "gdca_run_ranked_phased_async": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "gdca_run_ranked_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_run_ranked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_run_multi": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gdca_run_multi_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gdca_run_ranked_multi": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_energies_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "gdca_energies": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "gdca_run_energies_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                        C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_energies": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                    C.c_void_p, C.POINTER(Stats)]),
    "gdca_last_logdet": (C.c_int, [_ctx, C.c_int32, _f64p, _i32p]),
    "gdca_spd_inverse_logdet_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _i32p, _f64p]),
    "gdca_spd_inverse_logdet": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _i32p, _f64p]),
    "gdca_run_loglik_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                      C.c_void_p, _f64p, C.POINTER(Stats)]),
    "gdca_run_loglik": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                  C.c_void_p, _f64p, C.POINTER(Stats)]),
    "gdca_pair_energies_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_pair_energies": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_run_pair_energies_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_pair_energies": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(Stats)]),
    "gdca_pair_blocks_length": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int32]),
    "gdca_pair_energies_blocked_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_pair_energies_blocked": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_assign_blocks_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gdca_assign_blocks": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gdca_run_partner_match_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_partner_match": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_pair_logodds_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    "gdca_pair_logodds": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    "gdca_pair_logodds_blocked_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    "gdca_pair_logodds_blocked": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    "gdca_run_pair_logodds_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(Stats)]),
    "gdca_run_pair_logodds": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_partner_logodds_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                               C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_partner_logodds": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p,
                                           C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_select_confident_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, _i32p]),
    "gdca_select_confident": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, _i32p]),
    "gdca_concat_pairs_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_int32]),
    "gdca_concat_pairs": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_int32]),
    "gdca_run_partner_ipa_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32p,
                                           C.POINTER(Stats)]),
    "gdca_run_partner_ipa": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i32p,
                                       C.POINTER(Stats)]),
    "gdca_mutation_scan_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_mutation_scan": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_run_mutation_scan_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_mutation_scan": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_void_p, C.POINTER(Stats)]),
    "gdca_double_mutant_scan_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "gdca_double_mutant_scan": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "gdca_double_mutants_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p]),
    "gdca_double_mutants": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p]),
    "gdca_run_double_mutant_scan_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_double_mutant_scan": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_double_mutants_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_double_mutants": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Stats)]),
    "gdca_greedy_walk_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_greedy_walk": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                   C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_run_greedy_walk_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_greedy_walk": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_sample_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                                  C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "gdca_sample": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                              C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]),
    "gdca_run_sample_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_int32, C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_sample": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_int32, C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_sample_tempered_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "gdca_sample_tempered": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "gdca_run_sample_tempered_dev": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_run_sample_tempered": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Params), C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "gdca_log_partition_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_log_partition": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdca_potts_from_gaussian_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_potts_from_gaussian": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_bm_update_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                     C.c_double]),
    "gdca_bm_update": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                 C.c_double]),
    "gdca_bm_readout_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_bm_readout": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gdca_bm_learn_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                    C.c_void_p, C.c_void_p]),
    "gdca_bm_learn": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                C.c_void_p, C.c_void_p]),
    "gdca_plm_conditionals_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gdca_plm_conditionals": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gdca_plm_tally_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "gdca_plm_tally": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p]),
    "gdca_plm_tallies_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "gdca_plm_tallies": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "gdca_plm_learn_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p]),
    "gdca_plm_learn": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p]),
    "gdca_write_rank": (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "gdca_synth_family": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    "gdca_write_fasta": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]),
    "gdca_probe_mfma_f64": (C.c_int, [_ctx, C.c_int32, _f64p]),
}

_lib = None


def load() -> C.CDLL:
    """Load libgdca.so and bind every declared symbol.  Raises GdcaError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GdcaError(
            f"{LIB_PATH} not found: the HIP library has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    # the library writes sizeof(gdca_stats) bytes into the caller's struct: a build whose struct differs from this binding's
    # would overrun it (or leave fields unfilled) -- refuse it here instead (include/gdca.h, note at the end of gdca_stats)
    if lib.gdca_version() != ABI_VERSION or lib.gdca_stats_bytes() != C.sizeof(Stats) or lib.gdca_params_bytes() != C.sizeof(Params):
        raise GdcaError(f"{LIB_PATH} is version {lib.gdca_version()} with gdca_stats of {lib.gdca_stats_bytes()} bytes; this binding is "
                        f"written for version {ABI_VERSION} with {C.sizeof(Stats)} bytes: rebuild the library or update the binding")
    _lib = lib
    return lib


def _p(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def species_offsets(off) -> np.ndarray:
    """species offsets as the library takes them: a contiguous int32 vector of S + 1 >= 2 entries (its values are checked there)"""
    a = np.asarray(off)
    if a.ndim != 1 or a.size < 2 or not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > 2**31 - 1)):
        raise ArgumentError("species offsets must be a vector of S + 1 >= 2 non-negative integers")
    return np.ascontiguousarray(a, dtype=np.int32)


def pair_blocks_length(offA, offB) -> int:
    """gdca_pair_blocks_length: the doubles the packed blocked matrix of these species holds; -1 for invalid offsets"""
    offA, offB = np.ascontiguousarray(offA, dtype=np.int32), np.ascontiguousarray(offB, dtype=np.int32)
    if offA.ndim != 1 or offA.shape != offB.shape:
        return -1
    return int(load().gdca_pair_blocks_length(_p(offA), _p(offB), len(offA) - 1))


class Context:
    """One gdca_ctx = one HIP device + one stream + its workspace."""

    def __init__(self, device: int = 0, stream: int | None = None, _peer_of: "Context | None" = None):
        self.lib = load()
        h = _ctx()
        if _peer_of is not None:
            st = self.lib.gdca_ctx_create_peer(_peer_of.h, C.byref(h))
            device = _peer_of.device
        elif stream is None:
            st = self.lib.gdca_ctx_create(int(device), C.byref(h))
        else:
            st = self.lib.gdca_ctx_create_on_stream(int(device), C.c_void_p(stream), C.byref(h))
        if st != GDCA_OK:
            raise GdcaError(f"gdca_ctx_create(device={device}) failed with status {st}: no usable HIP device "
                            "(the gDCA hot path has no CPU fallback)")
        self.h = h
        self.device = int(device)

    def peer(self) -> "Context":
        """Another context on the same GPU whose inverse stages alternate with this one's (pipeline)."""
        return Context(_peer_of=self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gdca_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st: int, info: int = 0):
        if st == GDCA_OK:
            return
        msg = self.lib.gdca_last_error(self.h)
        msg = msg.decode() if msg else ""
        if st == GDCA_EINVAL:
            raise ArgumentError(msg or "invalid argument")
        if st == GDCA_ENOTPD:
            raise PosDefException(info)
        if st == GDCA_ENOMEM:
            raise MemoryError(msg)
        if st == GDCA_ENOCONV:
            raise ConvergenceError(-info if info < 0 else 0)
        raise GdcaError(f"HIP error: {msg}")

    def synchronize(self):
        self.check(self.lib.gdca_ctx_synchronize(self.h))

    def set_timing(self, on: bool):
        self.check(self.lib.gdca_ctx_set_timing(self.h, 1 if on else 0))

    def set_option(self, key: str, value) -> None:
        """Tuning switch of this context (gdca_ctx_set_option): key = a GDCA_* variable's name, with or without the prefix."""
        self.check(self.lib.gdca_ctx_set_option(self.h, str(key).encode(), str(value).encode()))

    def set_options(self, **kv) -> "Context":
        for k, v in kv.items():
            self.set_option(k, v)
        return self

    # ---- fused path ----
    def run(self, Zf: np.ndarray, q: int, pseudocount: float, theta: float, score: int, apc: bool = True):
        """Zf: int8, shape (N, M), Fortran-contiguous.  Returns (S[N,N], stats dict)."""
        N, M = Zf.shape
        S = np.empty((N, N), dtype=np.float64, order="F")  # (the library writes column-major; compute_ranking takes it as it is)
        prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
        st = Stats()
        rc = self.lib.gdca_run(self.h, _p(Zf), N, M, int(q), C.byref(prm), _p(S), C.byref(st))
        self.check(rc, st.info)
        return S, st.as_dict()

    def run_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, score: int, apc: bool = True):
        """gdca_run on a HOST matrix given by address (N x M int8, column-major: e.g. gdca_fasta_data).  Returns (S, stats)."""
        S = np.empty((N, N), dtype=np.float64, order="F")
        prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
        st = Stats()
        rc = self.lib.gdca_run(self.h, C.c_void_p(Z_ptr), int(N), int(M), int(q), C.byref(prm), _p(S), C.byref(st))
        self.check(rc, st.info)
        return S, st.as_dict()

    def run_ranked_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, score: int, min_separation: int,
                       apc: bool = True):
        """gdca_run_ranked on a HOST matrix given by address: src/GaussDCA.jl:28-44 in one call, the ranking is sorted on the
        device and only it comes back.  Returns (i, j, score, stats): int32, int32, float64 arrays."""
        n = max(int(self.lib.gdca_ranking_length(int(N), int(min_separation))), 0)
        ii = np.empty(n, dtype=np.int32)
        jj = np.empty(n, dtype=np.int32)
        sc = np.empty(n, dtype=np.float64)
        prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
        st = Stats()
        rc = self.lib.gdca_run_ranked(self.h, C.c_void_p(Z_ptr), int(N), int(M), int(q), C.byref(prm), int(min_separation), _p(ii), _p(jj),
                                      _p(sc), C.byref(st))
        self.check(rc, st.info)
        return ii, jj, sc, st.as_dict()

    # ---- read-outs of the fitted model: energies, pair energies, mutation scan ----
    @staticmethod
    def _opt(ptr):
        """an address as a void pointer; None (an optional argument left out) stays NULL"""
        return C.c_void_p(ptr) if ptr is not None else None

    def _run_readout(self, fn, Z_ptr, N, M, q, pseudocount, theta, *rest):
        """The frame of the fused read-outs: fn(ctx, Z, N, M, q, params, *rest, stats) with the read-outs' params (no contact score),
        checked.  Returns the stats dict."""
        prm = Params(float(pseudocount), float(theta), SCORE_FROB, 0)
        st = Stats()
        rc = fn(self.h, C.c_void_p(Z_ptr), int(N), int(M), int(q), C.byref(prm), *rest, C.byref(st))
        self.check(rc, st.info)
        return st.as_dict()

    # ---- energies of sequences under the fitted model (gdca_run_energies) ----
    def run_energies_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None = None, K: int = 0):
        """gdca_run_energies on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run() fits
        it, then E(x) = 1/2 (x - Pi)' mJ (x - Pi) of the K sequences X (N x K, same layout; None: Z's own M sequences).
        Returns (E float64[K], stats)."""
        Ke = int(K) if X_ptr is not None else int(M)
        E = np.empty(max(Ke, 0), dtype=np.float64)
        return E, self._run_readout(self.lib.gdca_run_energies, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K), _p(E))

    def run_energies_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None, K: int, E_ptr: int):
        """Device-pointer form (Z, X and E resident in HBM).  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_energies_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 C.c_void_p(E_ptr))

    # ---- log-likelihoods: log det C from the pivots of the inverse (include/gdca.h, "log-likelihoods") ----
    def last_logdet(self, k: int = 0, return_source: bool = False):
        """log det of the matrix of the last SPD inverse this context completed (gdca_last_logdet); k: the member index after
        run_multi; after a fused log-odds run 0 = the joint C, 1 = C_AA, 2 = C_BB.  NaN where that inverse was not positive definite.  return_source: (logdet, source), source 0 = the sweep's
        pivots, 1 = the Cholesky fallback's diagonal."""
        v = C.c_double(float("nan"))
        src = C.c_int32(0)
        self.check(self.lib.gdca_last_logdet(self.h, int(k), C.byref(v), C.byref(src)))
        return (v.value, src.value) if return_source else v.value

    def spd_inverse_logdet(self, A: np.ndarray):
        """gdca_spd_inverse_logdet on a host matrix (n x n float64; symmetric, so either memory order): returns (inverse, logdet).
        PosDefException as spd_inverse raises it."""
        A = np.array(A, dtype=np.float64, order="F")
        n = A.shape[0]
        info = C.c_int32(0)
        v = C.c_double(float("nan"))
        self.check(self.lib.gdca_spd_inverse_logdet(self.h, _p(A), int(n), C.byref(info), C.byref(v)), info.value)
        return A, v.value

    def spd_inverse_logdet_dev(self, A_ptr: int, n: int) -> float:
        """Device-pointer form: A (n x n, ld n) is inverted in place; returns logdet."""
        info = C.c_int32(0)
        v = C.c_double(float("nan"))
        self.check(self.lib.gdca_spd_inverse_logdet_dev(self.h, C.c_void_p(A_ptr), int(n), C.byref(info), C.byref(v)), info.value)
        return v.value

    def run_loglik_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None = None, K: int = 0):
        """gdca_run_loglik on HOST matrices given by address (as run_energies_ptr): log p(x) = -E(x) - 1/2 (n log 2 pi + log det C)
        of the K sequences X (None: Z's own M).  Returns (L float64[K], logdet, stats)."""
        Ke = int(K) if X_ptr is not None else int(M)
        L = np.empty(max(Ke, 0), dtype=np.float64)
        v = C.c_double(float("nan"))
        st = self._run_readout(self.lib.gdca_run_loglik, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K), _p(L), C.byref(v))
        return L, v.value, st

    def run_loglik(self, Zf: np.ndarray, q: int, pseudocount: float, theta: float, X: np.ndarray | None = None):
        """run_loglik_ptr on arrays: Zf int8 (N, M) Fortran-contiguous, X int8 (N, K) likewise or None."""
        N, M = Zf.shape
        if X is None:
            return self.run_loglik_ptr(Zf.ctypes.data, N, M, q, pseudocount, theta)
        X = np.asfortranarray(X, dtype=np.int8)
        return self.run_loglik_ptr(Zf.ctypes.data, N, M, q, pseudocount, theta, X.ctypes.data, X.shape[1])

    def run_loglik_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None, K: int, L_ptr: int):
        """Device-pointer form (Z, X and L resident in HBM).  Returns (logdet, stats)."""
        v = C.c_double(float("nan"))
        st = self._run_readout(self.lib.gdca_run_loglik_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                               C.c_void_p(L_ptr), C.byref(v))
        return v.value, st

    def energies_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, X_ptr: int, K: int, E_ptr: int) -> None:
        """gdca_energies_dev: mJ (n x n), Pi (n), X (N x K int8) and E (K) are device pointers."""
        self.check(self.lib.gdca_energies_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), C.c_void_p(X_ptr), int(K),
                                              C.c_void_p(E_ptr)))

    # ---- energies of every pairing across a split alignment (gdca_run_pair_energies) ----
    def run_pair_energies_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int,
                              XA_ptr: int | None = None, KA: int = 0, XB_ptr: int | None = None, KB: int = 0, what: int = 1):
        """gdca_run_pair_energies on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run()
        fits it, then E[a, b] of the pairings of the KA sequences XA (split x KA) with the KB sequences XB ((N - split) x KB); None:
        the halves of Z's own M sequences.  ``what``: PAIR_ENERGY or PAIR_COUPLING.  Returns (E float64 (KA, KB), stats)."""
        ka = int(KA) if XA_ptr is not None else int(M)
        kb = int(KB) if XB_ptr is not None else int(M)
        E = np.empty((max(ka, 0), max(kb, 0)), dtype=np.float64, order="F")
        return E, self._run_readout(self.lib.gdca_run_pair_energies, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr),
                                    int(KA), self._opt(XB_ptr), int(KB), int(what), _p(E))

    def run_pair_energies_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int, XA_ptr: int | None,
                              KA: int, XB_ptr: int | None, KB: int, what: int, E_ptr: int):
        """Device-pointer form (Z, XA, XB and E resident in HBM; E column-major KA x KB).  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_pair_energies_dev, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr),
                                 int(KA), self._opt(XB_ptr), int(KB), int(what), C.c_void_p(E_ptr))

    def pair_energies_dev(self, mJ_ptr: int, Pi_ptr: int | None, N: int, q: int, split: int, XA_ptr: int, KA: int, XB_ptr: int, KB: int,
                          what: int, E_ptr: int) -> None:
        """gdca_pair_energies_dev: mJ (n x n), Pi (n; None for PAIR_COUPLING), XA (split x KA int8), XB ((N - split) x KB int8) and E
        (KA x KB, column-major) are device pointers."""
        self.check(self.lib.gdca_pair_energies_dev(self.h, C.c_void_p(mJ_ptr), self._opt(Pi_ptr), int(N), int(q), int(split),
                                                   C.c_void_p(XA_ptr), int(KA), C.c_void_p(XB_ptr), int(KB), int(what), C.c_void_p(E_ptr)))

    # ---- partner matching per species: blocked pair energies and the assignment (gdca_run_partner_match) ----
    def pair_energies_blocked_dev(self, mJ_ptr: int, Pi_ptr: int | None, N: int, q: int, split: int, XA_ptr: int, KA: int, XB_ptr: int,
                                  KB: int, offA, offB, what: int, E_ptr: int) -> None:
        """gdca_pair_energies_blocked_dev: as pair_energies_dev for species-sorted sequences; offA / offB are HOST offsets (S + 1
        each), E the packed blocks (pair_blocks_length(offA, offB) doubles, device)."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        self.check(self.lib.gdca_pair_energies_blocked_dev(self.h, C.c_void_p(mJ_ptr), self._opt(Pi_ptr), int(N), int(q), int(split),
                                                           C.c_void_p(XA_ptr), int(KA), C.c_void_p(XB_ptr), int(KB), _p(offA), _p(offB),
                                                           len(offA) - 1, int(what), C.c_void_p(E_ptr)))

    def assign_blocks_dev(self, E_ptr: int, offA, offB, match_ptr: int, gap_ptr: int | None = None) -> None:
        """gdca_assign_blocks_dev: the minimum-cost assignment inside every block of the packed cost matrix E (device); match (int32,
        offA[-1] entries) and gap (float64, or None) are device pointers, offA / offB HOST offsets."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        self.check(self.lib.gdca_assign_blocks_dev(self.h, C.c_void_p(E_ptr), _p(offA), _p(offB), len(offA) - 1, C.c_void_p(match_ptr),
                                                   self._opt(gap_ptr)))

    def run_partner_match_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int, XA_ptr: int | None,
                              KA: int, XB_ptr: int | None, KB: int, offA, offB, what: int = 1, want_blocks: bool = True):
        """gdca_run_partner_match on HOST matrices given by address: the model is fitted on Z as run() fits it, then the blocked pair
        energies of the species-sorted XA / XB (None: that half of Z's own sequences) and the assignment inside every species.
        Returns ((E packed float64 or None, match int32[KA], gap float64[KA]), stats)."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        ka = int(KA) if XA_ptr is not None else int(M)
        E = np.empty(max(pair_blocks_length(offA, offB), 0), dtype=np.float64) if want_blocks else None
        match, gap = np.empty(max(ka, 0), dtype=np.int32), np.empty(max(ka, 0), dtype=np.float64)
        st = self._run_readout(self.lib.gdca_run_partner_match, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr), int(KA),
                               self._opt(XB_ptr), int(KB), _p(offA), _p(offB), len(offA) - 1, int(what), None if E is None else _p(E),
                               _p(match), _p(gap))
        return (E, match, gap), st

    def run_partner_match_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int, XA_ptr: int | None,
                              KA: int, XB_ptr: int | None, KB: int, offA, offB, what: int, E_ptr: int | None, match_ptr: int,
                              gap_ptr: int | None):
        """Device-pointer form (Z, XA, XB, E, match and gap resident in HBM; E None: kept inside the context).  Returns the stats dict."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        return self._run_readout(self.lib.gdca_run_partner_match_dev, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr),
                                 int(KA), self._opt(XB_ptr), int(KB), _p(offA), _p(offB), len(offA) - 1, int(what), self._opt(E_ptr),
                                 C.c_void_p(match_ptr), self._opt(gap_ptr))

    # ---- pair log-odds: the joint model against the two marginal models (include/gdca.h, "pair log-odds") ----
    def pair_logodds_dev(self, mJ_ptr: int, mJA_ptr: int, mJB_ptr: int, Pi_ptr: int, N: int, q: int, split: int, XA_ptr: int, KA: int,
                         XB_ptr: int, KB: int, I: float, L_ptr: int) -> None:
        """gdca_pair_logodds_dev: the three precisions (n x n, n_A x n_A, n_B x n_B), Pi (n), XA (split x KA int8), XB ((N - split) x KB
        int8) and L (KA x KB, column-major) are device pointers; I the caller's -1/2 (log det C - log det C_AA - log det C_BB)."""
        self.check(self.lib.gdca_pair_logodds_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(mJA_ptr), C.c_void_p(mJB_ptr), C.c_void_p(Pi_ptr),
                                                  int(N), int(q), int(split), C.c_void_p(XA_ptr), int(KA), C.c_void_p(XB_ptr), int(KB),
                                                  float(I), C.c_void_p(L_ptr)))

    def pair_logodds_blocked_dev(self, mJ_ptr: int, mJA_ptr: int, mJB_ptr: int, Pi_ptr: int, N: int, q: int, split: int, XA_ptr: int,
                                 KA: int, XB_ptr: int, KB: int, offA, offB, I: float, L_ptr: int) -> None:
        """gdca_pair_logodds_blocked_dev: as pair_logodds_dev for species-sorted sequences; offA / offB are HOST offsets, L the packed
        blocks (pair_blocks_length(offA, offB) doubles, device)."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        self.check(self.lib.gdca_pair_logodds_blocked_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(mJA_ptr), C.c_void_p(mJB_ptr),
                                                          C.c_void_p(Pi_ptr), int(N), int(q), int(split), C.c_void_p(XA_ptr), int(KA),
                                                          C.c_void_p(XB_ptr), int(KB), _p(offA), _p(offB), len(offA) - 1, float(I),
                                                          C.c_void_p(L_ptr)))

    def run_pair_logodds_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int,
                             XA_ptr: int | None = None, KA: int = 0, XB_ptr: int | None = None, KB: int = 0):
        """gdca_run_pair_logodds on HOST matrices given by address: the joint model and the two marginal models are fitted on Z (one
        front end, three inverses), then L[a, b] = log p_AB(a (+) b) - log p_A(a) - log p_B(b) of the pairings of XA (split x KA) with
        XB ((N - split) x KB); None: the halves of Z's own M sequences.  Returns ((L float64 (KA, KB), EmA float64[KA], EmB
        float64[KB], info dict by LOGODDS_FIELDS), stats of the joint fit)."""
        ka = int(KA) if XA_ptr is not None else int(M)
        kb = int(KB) if XB_ptr is not None else int(M)
        L = np.empty((max(ka, 0), max(kb, 0)), dtype=np.float64, order="F")
        EmA, EmB = np.empty(max(ka, 0), dtype=np.float64), np.empty(max(kb, 0), dtype=np.float64)
        info = np.zeros(len(LOGODDS_FIELDS), dtype=np.float64)
        st = self._run_readout(self.lib.gdca_run_pair_logodds, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr), int(KA),
                               self._opt(XB_ptr), int(KB), _p(L), _p(EmA), _p(EmB), _p(info))
        return (L, EmA, EmB, dict(zip(LOGODDS_FIELDS, info.tolist()))), st

    def run_pair_logodds_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int, XA_ptr: int | None,
                             KA: int, XB_ptr: int | None, KB: int, L_ptr: int, EmA_ptr: int | None = None, EmB_ptr: int | None = None):
        """Device-pointer form (Z, XA, XB, L and the optional EmA / EmB resident in HBM).  Returns (info dict, stats)."""
        info = np.zeros(len(LOGODDS_FIELDS), dtype=np.float64)
        st = self._run_readout(self.lib.gdca_run_pair_logodds_dev, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr),
                               int(KA), self._opt(XB_ptr), int(KB), C.c_void_p(L_ptr), self._opt(EmA_ptr), self._opt(EmB_ptr), _p(info))
        return dict(zip(LOGODDS_FIELDS, info.tolist())), st

    def run_partner_logodds_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int, XA_ptr: int | None,
                                KA: int, XB_ptr: int | None, KB: int, offA, offB, want_blocks: bool = True):
        """gdca_run_partner_logodds on HOST matrices given by address: run_pair_logodds_ptr's fits, then the blocked log-odds of the
        species-sorted XA / XB and the assignment that MAXIMISES their total inside every species.  Returns ((L packed float64 or None,
        match int32[KA], gap float64[KA], info dict), stats)."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        ka = int(KA) if XA_ptr is not None else int(M)
        L = np.empty(max(pair_blocks_length(offA, offB), 0), dtype=np.float64) if want_blocks else None
        match, gap = np.empty(max(ka, 0), dtype=np.int32), np.empty(max(ka, 0), dtype=np.float64)
        info = np.zeros(len(LOGODDS_FIELDS), dtype=np.float64)
        st = self._run_readout(self.lib.gdca_run_partner_logodds, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr), int(KA),
                               self._opt(XB_ptr), int(KB), _p(offA), _p(offB), len(offA) - 1, None if L is None else _p(L), _p(match),
                               _p(gap), _p(info))
        return (L, match, gap, dict(zip(LOGODDS_FIELDS, info.tolist()))), st

    def run_partner_logodds_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, split: int, XA_ptr: int | None,
                                KA: int, XB_ptr: int | None, KB: int, offA, offB, L_ptr: int | None, match_ptr: int, gap_ptr: int | None):
        """Device-pointer form (L None: kept inside the context).  Returns (info dict, stats)."""
        offA, offB = species_offsets(offA), species_offsets(offB)
        info = np.zeros(len(LOGODDS_FIELDS), dtype=np.float64)
        st = self._run_readout(self.lib.gdca_run_partner_logodds_dev, Z_ptr, N, M, q, pseudocount, theta, int(split), self._opt(XA_ptr),
                               int(KA), self._opt(XB_ptr), int(KB), _p(offA), _p(offB), len(offA) - 1, self._opt(L_ptr),
                               C.c_void_p(match_ptr), self._opt(gap_ptr), _p(info))
        return dict(zip(LOGODDS_FIELDS, info.tolist())), st

    # ---- iterative partner matching: the selection, the concatenation and the loop (gdca_run_partner_ipa) ----
    def select_confident(self, match: np.ndarray, gap: np.ndarray, n_take: int):
        """gdca_select_confident on host vectors (match int32[KA], gap float64[KA] as assign_blocks returns them): the first
        min(n_take, candidates) candidates by gap descending, ties in ascending a.  Returns (sel int32[KA]: the selected a ascending,
        then -1; n_sel)."""
        match, gap = np.ascontiguousarray(match, dtype=np.int32), np.ascontiguousarray(gap, dtype=np.float64)
        sel = np.empty(len(match), dtype=np.int32)
        n = C.c_int32(0)
        self.check(self.lib.gdca_select_confident(self.h, _p(match), _p(gap), len(match), int(n_take), _p(sel), C.byref(n)))
        return sel, n.value

    def select_confident_dev(self, match_ptr: int, gap_ptr: int, KA: int, n_take: int, sel_ptr: int) -> int:
        """Device-pointer form (match, gap and sel resident in HBM).  Returns n_sel."""
        n = C.c_int32(0)
        self.check(self.lib.gdca_select_confident_dev(self.h, C.c_void_p(match_ptr), C.c_void_p(gap_ptr), int(KA), int(n_take),
                                                      C.c_void_p(sel_ptr), C.byref(n)))
        return n.value

    def concat_pairs(self, XA: np.ndarray, XB: np.ndarray, selA, selB, Z: np.ndarray, col0: int = 0) -> None:
        """gdca_concat_pairs on host arrays: column col0 + t of Z (int8 (N, M), Fortran-contiguous, written in place) becomes
        XA[:, selA[t]] over XB[:, selB[t]]."""
        XA, XB = np.asfortranarray(XA, dtype=np.int8), np.asfortranarray(XB, dtype=np.int8)
        selA, selB = np.ascontiguousarray(selA, dtype=np.int32), np.ascontiguousarray(selB, dtype=np.int32)
        if len(selA) != len(selB) or Z.dtype != np.int8 or not Z.flags.f_contiguous or Z.shape[0] != XA.shape[0] + XB.shape[0] \
                or col0 < 0 or col0 + len(selA) > Z.shape[1]:
            raise ArgumentError("Z must be an int8 Fortran-contiguous (N, M) array with M >= col0 + len(selA), and len(selA) == len(selB)")
        self.check(self.lib.gdca_concat_pairs(self.h, _p(XA), XA.shape[1], _p(XB), XB.shape[1], Z.shape[0], XA.shape[0], _p(selA), _p(selB),
                                              len(selA), _p(Z), int(col0)))

    def concat_pairs_dev(self, XA_ptr: int, KA: int, XB_ptr: int, KB: int, N: int, split: int, selA_ptr: int, selB_ptr: int, n_sel: int,
                         Z_ptr: int, col0: int = 0) -> None:
        """Device-pointer form (the pools, the index vectors and Z resident in HBM)."""
        self.check(self.lib.gdca_concat_pairs_dev(self.h, C.c_void_p(XA_ptr), int(KA), C.c_void_p(XB_ptr), int(KB), int(N), int(split),
                                                  C.c_void_p(selA_ptr), C.c_void_p(selB_ptr), int(n_sel), C.c_void_p(Z_ptr), int(col0)))

    def _ipa(self, fn, XA_ptr, KA, XB_ptr, KB, offA, offB, N, q, split, what, pseudocount, theta, Zfix_ptr, Mfix, seedA, seedB, n_inc,
             max_rounds, match_p, gap_p, mt_p, gt_p):
        offA, offB = species_offsets(offA), species_offsets(offB)
        seedA, seedB = np.ascontiguousarray(seedA, dtype=np.int32), np.ascontiguousarray(seedB, dtype=np.int32)
        if seedA.ndim != 1 or seedA.shape != seedB.shape:
            raise ArgumentError("the seed must be two index vectors of one length")
        prm = Params(float(pseudocount), float(theta), SCORE_FROB, 0)
        st = Stats()
        rounds = np.zeros((max(int(max_rounds), 1), len(IPA_FIELDS)), dtype=np.float64)
        done = C.c_int32(0)
        rc = fn(self.h, self._opt(XA_ptr), int(KA), self._opt(XB_ptr), int(KB), _p(offA), _p(offB), len(offA) - 1, int(N), int(q), int(split),
                int(what), C.byref(prm), self._opt(Zfix_ptr), int(Mfix), _p(seedA), _p(seedB), len(seedA), int(n_inc), int(max_rounds),
                match_p, gap_p, mt_p, gt_p, _p(rounds), C.byref(done), C.byref(st))
        self.rounds_run = done.value   # (kept where the call raises: the completed rounds' results are in the caller's arrays)
        self.check(rc, st.info)
        return [dict(zip(IPA_FIELDS, row.tolist())) for row in rounds[:done.value]], st.as_dict()

    def run_partner_ipa_ptr(self, XA_ptr: int, KA: int, XB_ptr: int, KB: int, offA, offB, N: int, q: int, split: int, pseudocount: float,
                            theta: float, Zfix_ptr: int | None, Mfix: int, seedA, seedB, n_inc: int, max_rounds: int, what: int = 1,
                            want_traces: bool = False):
        """gdca_run_partner_ipa on HOST matrices given by address: the species-sorted pools XA (split x KA) and XB ((N - split) x KB),
        Zfix (N x Mfix, or None) and the seed (index pairs into the pools).  Returns ((match int32[KA], gap float64[KA], match_trace,
        gap_trace -- (rounds, KA) arrays or None), rounds: one dict a completed round (IPA_FIELDS), stats of the last fit)."""
        ka = max(int(KA), 0)
        match, gap = np.empty(ka, dtype=np.int32), np.empty(ka, dtype=np.float64)
        mt = np.empty((max(int(max_rounds), 1), ka), dtype=np.int32) if want_traces else None
        gt = np.empty((max(int(max_rounds), 1), ka), dtype=np.float64) if want_traces else None
        rounds, st = self._ipa(self.lib.gdca_run_partner_ipa, XA_ptr, KA, XB_ptr, KB, offA, offB, N, q, split, what, pseudocount, theta, Zfix_ptr,
                               Mfix, seedA, seedB, n_inc, max_rounds, _p(match), _p(gap), None if mt is None else _p(mt),
                               None if gt is None else _p(gt))
        if want_traces:
            mt, gt = mt[:len(rounds)], gt[:len(rounds)]
        return (match, gap, mt, gt), rounds, st

    def run_partner_ipa_dev(self, XA_ptr: int, KA: int, XB_ptr: int, KB: int, offA, offB, N: int, q: int, split: int, pseudocount: float,
                            theta: float, Zfix_ptr: int | None, Mfix: int, seedA, seedB, n_inc: int, max_rounds: int, what: int,
                            match_ptr: int, gap_ptr: int | None, match_trace_ptr: int | None = None, gap_trace_ptr: int | None = None):
        """Device-pointer form (the pools, Zfix, match, gap and the traces resident in HBM; the seed and the offsets are host arrays).
        Returns (rounds, stats)."""
        return self._ipa(self.lib.gdca_run_partner_ipa_dev, XA_ptr, KA, XB_ptr, KB, offA, offB, N, q, split, what, pseudocount, theta, Zfix_ptr,
                         Mfix, seedA, seedB, n_inc, max_rounds, C.c_void_p(match_ptr), self._opt(gap_ptr), self._opt(match_trace_ptr),
                         self._opt(gap_trace_ptr))

    # ---- the energy change of every single substitution (gdca_run_mutation_scan) ----
    def run_mutation_scan_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None = None,
                              K: int = 0, what: int = 0):
        """gdca_run_mutation_scan on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run() fits
        it, then D[k, i, b - 1] = the energy change of setting site i of sequence k of X (N x K, same layout; None: Z's own M sequences)
        to symbol b (``what`` = MUT_DELTA), or the site potential V (MUT_POTENTIAL).  Returns (D float64 (K, N, q), stats)."""
        Ke = int(K) if X_ptr is not None else int(M)
        D = np.empty((max(Ke, 0), int(N), int(q)), dtype=np.float64)
        return D, self._run_readout(self.lib.gdca_run_mutation_scan, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                    int(what), _p(D))

    def run_mutation_scan_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None, K: int,
                              what: int, D_ptr: int):
        """Device-pointer form (Z, X and D resident in HBM; D holds q N K doubles).  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_mutation_scan_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 int(what), C.c_void_p(D_ptr))

    def mutation_scan_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, X_ptr: int, K: int, what: int, D_ptr: int) -> None:
        """gdca_mutation_scan_dev: mJ (n x n), Pi (n), X (N x K int8) and D (q N K doubles, (K, N, q) row-major) are device pointers."""
        self.check(self.lib.gdca_mutation_scan_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), C.c_void_p(X_ptr), int(K),
                                                   int(what), C.c_void_p(D_ptr)))

    # ---- double mutants: the best double substitution and the epistasis of every site pair, listed double mutants ----
    def run_double_mutant_scan_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int, K: int):
        """gdca_run_double_mutant_scan on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run()
        fits it, then the three maps of the K sequences X (N x K, same layout; required).  Returns ((Emin float64 (K, N, N), code int32
        (K, N, N), epi float64 (K, N, N)), stats); entry [k, j, i] of the row-major arrays is [i, j, k] of include/gdca.h."""
        shape = (max(int(K), 0), int(N), int(N))
        Emin, code, epi = np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.int32), np.empty(shape, dtype=np.float64)
        st = self._run_readout(self.lib.gdca_run_double_mutant_scan, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K), _p(Emin),
                               _p(code), _p(epi))
        return (Emin, code, epi), st

    def run_double_mutant_scan_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int, K: int,
                                   Emin_ptr: int | None, code_ptr: int | None, epi_ptr: int | None):
        """Device-pointer form (Z, X and the maps resident in HBM; a map given as None is skipped).  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_double_mutant_scan_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 self._opt(Emin_ptr), self._opt(code_ptr), self._opt(epi_ptr))

    def run_double_mutants_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int, K: int,
                               muts_ptr: int, L: int):
        """gdca_run_double_mutants on HOST arrays given by address: muts holds L records (k, i, b, j, c) of int32, 5 x L column-major.
        Returns (ddE float64 (L,), stats)."""
        out = np.empty(max(int(L), 0), dtype=np.float64)
        return out, self._run_readout(self.lib.gdca_run_double_mutants, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                      self._opt(muts_ptr), int(L), _p(out))

    def run_double_mutants_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int, K: int,
                               muts_ptr: int, L: int, out_ptr: int):
        """Device-pointer form.  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_double_mutants_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 self._opt(muts_ptr), int(L), self._opt(out_ptr))

    def double_mutant_scan_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, X_ptr: int | None, K: int, Emin_ptr: int | None,
                               code_ptr: int | None, epi_ptr: int | None) -> None:
        """gdca_double_mutant_scan_dev: mJ (n x n), Pi (n), X (N x K int8) and the maps (N N K entries each; None: skipped) are device
        pointers."""
        self.check(self.lib.gdca_double_mutant_scan_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), self._opt(X_ptr), int(K),
                                                        self._opt(Emin_ptr), self._opt(code_ptr), self._opt(epi_ptr)))

    def double_mutants_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, X_ptr: int | None, K: int, muts_ptr: int | None, L: int,
                           out_ptr: int | None) -> None:
        """gdca_double_mutants_dev: muts (5 x L int32) and out (L doubles) are device pointers like the rest."""
        self.check(self.lib.gdca_double_mutants_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), self._opt(X_ptr), int(K),
                                                    self._opt(muts_ptr), int(L), self._opt(out_ptr)))

    # ---- greedy walk: every sequence descends to a local energy minimum (gdca_greedy_walk*, gdca_run_greedy_walk*) ----
    def greedy_walk_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, X_ptr: int | None, K: int, mask_ptr: int | None, flags: int,
                        min_gain: float, max_steps: int, Xout_ptr: int | None, steps_ptr: int | None, dE_sum_ptr: int | None = None,
                        path_ptr: int | None = None, dE_path_ptr: int | None = None, V_ptr: int | None = None) -> None:
        """gdca_greedy_walk_dev: mJ (n x n), Pi (n), X (N x K int8), mask (N int8 or None) and the outputs -- Xout (N x K int8), steps
        (K int32), dE_sum (K f64), path (2 x max_steps x K int32), dE_path (max_steps x K f64), V (q N K f64); the last four may be
        None -- are device pointers."""
        self.check(self.lib.gdca_greedy_walk_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), self._opt(X_ptr), int(K),
                                                 self._opt(mask_ptr), int(flags), float(min_gain), int(max_steps), self._opt(Xout_ptr),
                                                 self._opt(steps_ptr), self._opt(dE_sum_ptr), self._opt(path_ptr), self._opt(dE_path_ptr),
                                                 self._opt(V_ptr)))

    def run_greedy_walk_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None, K: int,
                            mask_ptr: int | None, flags: int, min_gain: float, max_steps: int, Xout_ptr: int | None, steps_ptr: int | None,
                            dE_sum_ptr: int | None = None, path_ptr: int | None = None, dE_path_ptr: int | None = None,
                            V_ptr: int | None = None):
        """gdca_run_greedy_walk_dev: the model is fitted on Z (N x M int8 in HBM) as run() fits it, then the walk of X (None: Z's own M
        sequences); the outputs as greedy_walk_dev's.  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_greedy_walk_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 self._opt(mask_ptr), int(flags), float(min_gain), int(max_steps), self._opt(Xout_ptr), self._opt(steps_ptr),
                                 self._opt(dE_sum_ptr), self._opt(path_ptr), self._opt(dE_path_ptr), self._opt(V_ptr))

    @staticmethod
    def walk_outputs(N: int, K: int, q: int, max_steps: int, path: bool, table: bool):
        """the host arrays a walk of K sequences fills, in the library's memory order: (Xout (N, K) Fortran int8, steps, dE_sum,
        path (K, max_steps, 2) int32 or None, dE_path (K, max_steps) or None, V (K, N, q) or None)"""
        K, T = max(int(K), 0), max(int(max_steps), 0)
        return (np.empty((int(N), K), dtype=np.int8, order="F"), np.empty(K, dtype=np.int32), np.empty(K, dtype=np.float64),
                np.empty((K, T, 2), dtype=np.int32) if path else None, np.empty((K, T), dtype=np.float64) if path else None,
                np.empty((K, int(N), int(q)), dtype=np.float64) if table else None)

    @staticmethod
    def walk_result(out):
        """(Xout, steps, dE_sum[, path, dE_path][, V]): the arrays of walk_outputs that were asked for"""
        Xout, steps, dE_sum, pth, dpth, V = out
        return (Xout, steps, dE_sum) + ((pth, dpth) if pth is not None else ()) + ((V,) if V is not None else ())

    def run_greedy_walk_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None = None, K: int = 0,
                            mask: np.ndarray | None = None, flags: int = 0, min_gain: float = 0.0, max_steps: int = 1, path: bool = False,
                            table: bool = False):
        """gdca_run_greedy_walk on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run() fits it,
        then the K sequences X (N x K, same layout; None: Z's own M sequences) walk to their local minima.  mask: N int8 or None.
        Returns ((Xout (N, K), steps (K,), dE_sum (K,)[, path (K, max_steps, 2), dE_path (K, max_steps)][, V (K, N, q)]), stats)."""
        Ke = int(K) if X_ptr is not None else int(M)
        out = self.walk_outputs(N, Ke, q, max_steps, path, table)
        opt = lambda a: None if a is None else _p(a)  # noqa: E731
        st = self._run_readout(self.lib.gdca_run_greedy_walk, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K), opt(mask), int(flags),
                               float(min_gain), int(max_steps), *[opt(a) for a in out])
        return self.walk_result(out), st

    # ---- Metropolis chains: sequences drawn from the model at an inverse temperature (gdca_sample*, gdca_run_sample*) ----
    def sample_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, X_ptr: int | None, K: int, mask_ptr: int | None, flags: int, beta: float,
                   seed: int, stream0: int, burn: int, stride: int, n_samples: int, Xs_ptr: int | None, accepted_ptr: int | None,
                   dE_s_ptr: int | None = None, thr_ptr: int | None = None, moves_ptr: int | None = None, V_ptr: int | None = None) -> None:
        """gdca_sample_dev: mJ (n x n), Pi (n), X (N x K int8), mask (N int8 or None) and the outputs -- Xs (N x n_samples x K int8),
        accepted (K int32), dE_s (n_samples x K f64), thr (n_steps x K f64), moves (n_steps x K int32), V (q N K f64); the last four
        may be None -- are device pointers."""
        self.check(self.lib.gdca_sample_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), self._opt(X_ptr), int(K),
                                            self._opt(mask_ptr), int(flags), float(beta), int(seed), int(stream0), int(burn), int(stride),
                                            int(n_samples), self._opt(Xs_ptr), self._opt(dE_s_ptr), self._opt(accepted_ptr),
                                            self._opt(thr_ptr), self._opt(moves_ptr), self._opt(V_ptr)))

    def run_sample_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None, K: int,
                       mask_ptr: int | None, flags: int, beta: float, seed: int, stream0: int, burn: int, stride: int, n_samples: int,
                       Xs_ptr: int | None, accepted_ptr: int | None, dE_s_ptr: int | None = None, thr_ptr: int | None = None,
                       moves_ptr: int | None = None, V_ptr: int | None = None):
        """gdca_run_sample_dev: the model is fitted on Z (N x M int8 in HBM) as run() fits it, then the chains from X (None: one from
        each of Z's own M sequences); the outputs as sample_dev's.  Returns the stats dict."""
        return self._run_readout(self.lib.gdca_run_sample_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 self._opt(mask_ptr), int(flags), float(beta), int(seed), int(stream0), int(burn), int(stride),
                                 int(n_samples), self._opt(Xs_ptr), self._opt(dE_s_ptr), self._opt(accepted_ptr), self._opt(thr_ptr),
                                 self._opt(moves_ptr), self._opt(V_ptr))

    @staticmethod
    def sample_outputs(N: int, K: int, q: int, burn: int, stride: int, n_samples: int, trace: bool, table: bool):
        """the host arrays the chains of K start sequences fill, in the library's memory order: (Xs (N, n_samples, K) Fortran int8, dE_s
        (K, n_samples), accepted (K,) int32, thr (K, n_steps) or None, moves (K, n_steps) int32 or None, V (K, N, q) or None)"""
        K, S = max(int(K), 0), max(int(n_samples), 0)
        T = max(int(burn) + S * int(stride), 0)
        return (np.empty((int(N), S, K), dtype=np.int8, order="F"), np.empty((K, S), dtype=np.float64), np.empty(K, dtype=np.int32),
                np.empty((K, T), dtype=np.float64) if trace else None, np.empty((K, T), dtype=np.int32) if trace else None,
                np.empty((K, int(N), int(q)), dtype=np.float64) if table else None)

    @staticmethod
    def sample_result(out):
        """(Xs, dE_s, accepted[, thr, moves][, V]): the arrays of sample_outputs that were asked for"""
        Xs, dE_s, acc, thr, moves, V = out
        return (Xs, dE_s, acc) + ((thr, moves) if thr is not None else ()) + ((V,) if V is not None else ())

    def run_sample_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None = None, K: int = 0,
                       mask: np.ndarray | None = None, flags: int = 0, beta: float = 1.0, seed: int = 0, stream0: int = 0, burn: int = 0,
                       stride: int = 1, n_samples: int = 1, trace: bool = False, table: bool = False):
        """gdca_run_sample on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run() fits it, then
        one Metropolis chain starts from each of the K sequences X (N x K, same layout; None: Z's own M sequences).  mask: N int8 or
        None.  Returns ((Xs (N, n_samples, K), dE_s (K, n_samples), accepted (K,)[, thr (K, n_steps), moves (K, n_steps)][, V (K, N, q)]),
        stats)."""
        Ke = int(K) if X_ptr is not None else int(M)
        out = self.sample_outputs(N, Ke, q, burn, stride, n_samples, trace, table)
        opt = lambda a: None if a is None else _p(a)  # noqa: E731
        st = self._run_readout(self.lib.gdca_run_sample, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K), opt(mask), int(flags),
                               float(beta), int(seed), int(stream0), int(burn), int(stride), int(n_samples), *[opt(a) for a in out])
        return self.sample_result(out), st

    # ---- replica-exchange chains: the Metropolis chains tempered over a ladder (gdca_sample_tempered*, gdca_run_sample_tempered*) ----
    @staticmethod
    def _betas(betas):
        """the ladder as the library takes it: a HOST array of R f64 (kept alive by the caller for the call)"""
        return np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)

    def sample_tempered_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, Xr_ptr: int | None, slot0_ptr: int | None, K: int, betas,
                            mask_ptr: int | None, flags: int, seed: int, stream0: int, swap_every: int, burn: int, stride: int, n_samples: int,
                            Xs_ptr: int | None, accepted_ptr: int | None, swaps_ptr: int | None, Xr_out_ptr: int | None,
                            slot_out_ptr: int | None, E_s_ptr: int | None = None, thr_ptr: int | None = None, moves_ptr: int | None = None,
                            swap_thr_ptr: int | None = None, slot_path_ptr: int | None = None) -> None:
        """gdca_sample_tempered_dev: mJ (n x n), Pi (n), Xr (N x R x K int8), slot0 (R x K int32 or None), mask (N int8 or None) and
        the outputs -- Xs (N x n_samples x K int8), accepted (R x K int32), swaps ((R - 1) x K int32), Xr_out (N x R x K int8), slot_out
        (R x K int32), E_s (n_samples x K f64), thr / moves (n_steps x R x K), swap_thr (n_rounds x (R - 1) x K f64), slot_path
        (n_rounds x R x K int32); the last five may be None -- are device pointers; betas (R values, betas[0] the target) is a host
        sequence."""
        b = self._betas(betas)
        self.check(self.lib.gdca_sample_tempered_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), self._opt(Xr_ptr),
                                                     self._opt(slot0_ptr), int(K), int(b.size), _p(b), self._opt(mask_ptr), int(flags), int(seed),
                                                     int(stream0), int(swap_every), int(burn), int(stride), int(n_samples), self._opt(Xs_ptr),
                                                     self._opt(E_s_ptr), self._opt(accepted_ptr), self._opt(swaps_ptr), self._opt(Xr_out_ptr),
                                                     self._opt(slot_out_ptr), self._opt(thr_ptr), self._opt(moves_ptr), self._opt(swap_thr_ptr),
                                                     self._opt(slot_path_ptr)))

    def run_sample_tempered_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None, K: int, betas,
                                mask_ptr: int | None, flags: int, seed: int, stream0: int, swap_every: int, burn: int, stride: int,
                                n_samples: int, Xs_ptr: int | None, accepted_ptr: int | None, swaps_ptr: int | None, Xr_out_ptr: int | None,
                                slot_out_ptr: int | None, E_s_ptr: int | None = None, thr_ptr: int | None = None,
                                moves_ptr: int | None = None, swap_thr_ptr: int | None = None, slot_path_ptr: int | None = None):
        """gdca_run_sample_tempered_dev: the model is fitted on Z (N x M int8 in HBM) as run() fits it, then the tempered chains from X
        (N x K; None: one from each of Z's own M sequences), every replica of a chain at its chain's sequence; the outputs as
        sample_tempered_dev's.  Returns the stats dict."""
        b = self._betas(betas)
        return self._run_readout(self.lib.gdca_run_sample_tempered_dev, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K),
                                 int(b.size), _p(b), self._opt(mask_ptr), int(flags), int(seed), int(stream0), int(swap_every), int(burn),
                                 int(stride), int(n_samples), self._opt(Xs_ptr), self._opt(E_s_ptr), self._opt(accepted_ptr),
                                 self._opt(swaps_ptr), self._opt(Xr_out_ptr), self._opt(slot_out_ptr), self._opt(thr_ptr), self._opt(moves_ptr),
                                 self._opt(swap_thr_ptr), self._opt(slot_path_ptr))

    @staticmethod
    def tempered_outputs(N: int, K: int, R: int, swap_every: int, burn: int, stride: int, n_samples: int, trace: bool):
        """the host arrays K tempered chains of R replicas fill, in the library's memory order: (Xs (N, n_samples, K) Fortran int8, E_s
        (K, n_samples), accepted (K, R) int32, swaps (K, R - 1) int32, Xr_out (N, R, K) Fortran int8, slot_out (K, R) int32, then -- or
        None each -- thr (K, R, n_steps), moves (K, R, n_steps) int32, swap_thr (K, R - 1, n_rounds), slot_path (K, R, n_rounds) int32)"""
        K, R, S = max(int(K), 0), max(int(R), 1), max(int(n_samples), 0)
        T = max(int(burn) + S * int(stride), 0)
        E = T // max(int(swap_every), 1)
        return (np.empty((int(N), S, K), dtype=np.int8, order="F"), np.empty((K, S), dtype=np.float64), np.empty((K, R), dtype=np.int32),
                np.empty((K, R - 1), dtype=np.int32), np.empty((int(N), R, K), dtype=np.int8, order="F"), np.empty((K, R), dtype=np.int32),
                np.empty((K, R, T), dtype=np.float64) if trace else None, np.empty((K, R, T), dtype=np.int32) if trace else None,
                np.empty((K, R - 1, E), dtype=np.float64) if trace else None, np.empty((K, R, E), dtype=np.int32) if trace else None)

    @staticmethod
    def _swaps_arg(swaps):
        """swaps may not be NULL even where it is empty (R == 1)"""
        return _p(swaps) if swaps.size else _p(_NO_SWAPS)

    def run_sample_tempered_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, X_ptr: int | None = None, K: int = 0,
                                betas=(1.0,), mask: np.ndarray | None = None, flags: int = 0, seed: int = 0, stream0: int = 0,
                                swap_every: int = 1, burn: int = 0, stride: int = 1, n_samples: int = 1, trace: bool = False):
        """gdca_run_sample_tempered on HOST matrices given by address: the model is fitted on Z (N x M int8, column-major) as run() fits
        it, then K tempered chains start from the sequences X (N x K, same layout; None: Z's own M sequences).  Returns (the arrays of
        tempered_outputs, without the four traces unless trace), stats)."""
        Ke = int(K) if X_ptr is not None else int(M)
        b = self._betas(betas)
        out = self.tempered_outputs(N, Ke, b.size, swap_every, burn, stride, n_samples, trace)
        opt = lambda a: None if a is None or a.size == 0 else _p(a)  # noqa: E731
        ptrs = [opt(a) for a in out]
        ptrs[3] = self._swaps_arg(out[3])
        st = self._run_readout(self.lib.gdca_run_sample_tempered, Z_ptr, N, M, q, pseudocount, theta, self._opt(X_ptr), int(K), int(b.size),
                               _p(b), None if mask is None else _p(mask), int(flags), int(seed), int(stream0), int(swap_every), int(burn),
                               int(stride), int(n_samples), *ptrs)
        return tuple(a for a in out if a is not None), st

    # ---- log partition function by annealed importance sampling (gdca_log_partition*) ----
    def log_partition_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, x_ptr: int | None, mask_ptr: int | None, flags: int, betas,
                          sweep: int, K: int, seed: int, stream0: int, out4_ptr: int | None, logw_ptr: int | None,
                          E_end_ptr: int | None = None, X0_ptr: int | None = None, Xout_ptr: int | None = None,
                          accepted_ptr: int | None = None, thr_ptr: int | None = None, moves_ptr: int | None = None) -> None:
        """gdca_log_partition_dev: mJ (n x n), Pi (n), the template x (N int8 or None: every site is free), mask (N int8 or None) and
        the outputs -- out4 (4 f64: log Z, the effective sample size, max logw, log |Omega|), logw (K f64), E_end (K f64), X0 and Xout
        (N x K int8), accepted (K int32), thr / moves (n_steps x K); the last six may be None -- are device pointers; betas (L + 1
        values, betas[0] == 0, betas[L] the target) is a host sequence."""
        b = self._betas(betas)
        self.check(self.lib.gdca_log_partition_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), self._opt(x_ptr),
                                                   self._opt(mask_ptr), int(flags), _p(b), int(b.size) - 1, int(sweep), int(K), int(seed),
                                                   int(stream0), self._opt(out4_ptr), self._opt(logw_ptr), self._opt(E_end_ptr),
                                                   self._opt(X0_ptr), self._opt(Xout_ptr), self._opt(accepted_ptr), self._opt(thr_ptr),
                                                   self._opt(moves_ptr)))

    @staticmethod
    def log_partition_outputs(N: int, K: int, n_steps: int, trace: bool):
        """the host arrays the annealed chains fill, in the library's memory order: (out4 (4,), logw (K,), then -- or None each -- E_end
        (K,), X0 (N, K) Fortran int8, Xout (N, K) Fortran int8, accepted (K,) int32, thr (K, n_steps), moves (K, n_steps) int32)"""
        K, T = max(int(K), 0), max(int(n_steps), 0)
        if not trace:
            return (np.empty(4), np.empty(K)) + (None,) * 6
        return (np.empty(4), np.empty(K), np.empty(K), np.empty((int(N), K), dtype=np.int8, order="F"),
                np.empty((int(N), K), dtype=np.int8, order="F"), np.empty(K, dtype=np.int32), np.empty((K, T)), np.empty((K, T), dtype=np.int32))

    # ---- Boltzmann-machine refinement of the Potts model (W, zeros) the chains draw from (gdca_potts_from_gaussian*, gdca_bm_*) ----
    def potts_from_gaussian_dev(self, mJ_ptr: int, Pi_ptr: int, N: int, q: int, W_ptr: int) -> None:
        """gdca_potts_from_gaussian_dev: mJ (n x n), Pi (n) -> W (n x n; not mJ), device pointers"""
        self.check(self.lib.gdca_potts_from_gaussian_dev(self.h, C.c_void_p(mJ_ptr), C.c_void_p(Pi_ptr), int(N), int(q), C.c_void_p(W_ptr)))

    def bm_update_dev(self, W_ptr: int, Pij_d_ptr: int, Pij_m_ptr: int, N: int, q: int, eta: float, lam: float = 0.0,
                      Pi_d_ptr: int | None = None, Pi_m_ptr: int | None = None) -> None:
        """gdca_bm_update_dev: one gradient step on W (n x n) in place from the data's and the model's Pij (n x n), device pointers"""
        self.check(self.lib.gdca_bm_update_dev(self.h, C.c_void_p(W_ptr), self._opt(Pi_d_ptr), C.c_void_p(Pij_d_ptr), self._opt(Pi_m_ptr),
                                               C.c_void_p(Pij_m_ptr), int(N), int(q), float(eta), float(lam)))

    def bm_readout_dev(self, Pi_d_ptr: int, Pij_d_ptr: int, Pi_m_ptr: int, Pij_m_ptr: int, N: int, q: int, out4_ptr: int) -> None:
        """gdca_bm_readout_dev: the fit of the model's tallies to the data's in four f64 at out4 (a device pointer like the rest)"""
        self.check(self.lib.gdca_bm_readout_dev(self.h, C.c_void_p(Pi_d_ptr), C.c_void_p(Pij_d_ptr), C.c_void_p(Pi_m_ptr),
                                                C.c_void_p(Pij_m_ptr), int(N), int(q), C.c_void_p(out4_ptr)))

    def bm_learn_dev(self, W_ptr: int, Pi_d_ptr: int, Pij_d_ptr: int, N: int, q: int, X_ptr: int, K: int, mask_ptr: int | None, flags: int,
                     beta: float, seed: int, iter0: int, n_iter: int, burn: int, stride: int, n_samples: int, eta: float, lam: float,
                     trace_ptr: int, Xs_last_ptr: int | None = None) -> None:
        """gdca_bm_learn_dev: n_iter iterations of sample, tally, read out, update on W (n x n) and the chains X (N x K int8), both
        in place; trace (4 x n_iter f64) and the optional Xs_last (N x n_samples x K int8) are device pointers like the rest."""
        self.check(self.lib.gdca_bm_learn_dev(self.h, C.c_void_p(W_ptr), C.c_void_p(Pi_d_ptr), C.c_void_p(Pij_d_ptr), int(N), int(q),
                                              self._opt(X_ptr), int(K), self._opt(mask_ptr), int(flags), float(beta), int(seed), int(iter0),
                                              int(n_iter), int(burn), int(stride), int(n_samples), float(eta), float(lam),
                                              self._opt(trace_ptr), self._opt(Xs_last_ptr)))

    # ---- pseudo-likelihood fit of the Potts model (W, zeros) (gdca_plm_*): every argument a device pointer ----
    def plm_conditionals_dev(self, W_ptr: int, Z_ptr: int, N: int, M: int, q: int, p_ptr: int, nll_k_ptr: int) -> None:
        """gdca_plm_conditionals_dev: W (n x n), Z (N x M int8) -> p (q N M f64, the scan's layout) and nll_k (M)"""
        self.check(self.lib.gdca_plm_conditionals_dev(self.h, self._opt(W_ptr), self._opt(Z_ptr), int(N), int(M), int(q), self._opt(p_ptr),
                                                      self._opt(nll_k_ptr)))

    def plm_tally_dev(self, p_ptr: int, Z_ptr: int, w_ptr: int, Meff: float, N: int, M: int, q: int, Pi_c_ptr: int, Pij_c_ptr: int) -> None:
        """gdca_plm_tally_dev: the conditionals p, Z and the weights w (M) -> the conditional tallies Pi_c (n), Pij_c (n x n)"""
        self.check(self.lib.gdca_plm_tally_dev(self.h, self._opt(p_ptr), self._opt(Z_ptr), self._opt(w_ptr), float(Meff), int(N), int(M), int(q),
                                               self._opt(Pi_c_ptr), self._opt(Pij_c_ptr)))

    def plm_tallies_dev(self, W_ptr: int, Z_ptr: int, w_ptr: int, Meff: float, N: int, M: int, q: int, Pi_c_ptr: int, Pij_c_ptr: int,
                        nll_ptr: int) -> None:
        """gdca_plm_tallies_dev: the two above fused over slabs -> Pi_c, Pij_c and nll (one f64)"""
        self.check(self.lib.gdca_plm_tallies_dev(self.h, self._opt(W_ptr), self._opt(Z_ptr), self._opt(w_ptr), float(Meff), int(N), int(M),
                                                 int(q), self._opt(Pi_c_ptr), self._opt(Pij_c_ptr), self._opt(nll_ptr)))

    def plm_learn_dev(self, W_ptr: int, Z_ptr: int, w_ptr: int, Meff: float, Pi_d_ptr: int, Pij_d_ptr: int, N: int, M: int, q: int,
                      n_iter: int, eta: float, lam: float, trace_ptr: int) -> None:
        """gdca_plm_learn_dev: n_iter iterations of tallies, read-out (trace, 4 x n_iter f64, the fourth nll), step on W in place"""
        self.check(self.lib.gdca_plm_learn_dev(self.h, self._opt(W_ptr), self._opt(Z_ptr), self._opt(w_ptr), float(Meff), self._opt(Pi_d_ptr),
                                               self._opt(Pij_d_ptr), int(N), int(M), int(q), int(n_iter), float(eta), float(lam),
                                               self._opt(trace_ptr)))

    # ---- several settings of one alignment (gdca_run_multi): one front end, a covariance + inverse per distinct pseudocount ----
    def _check_multi(self, rc: int, sts, results):
        """Raise as check() does for the first failing member (its info); the exception carries every member's result in
        `.results` (a failing member's arrays are unspecified) and the members' statuses in `.statuses`."""
        if rc == GDCA_OK:
            return
        info = 0
        statuses = []
        for st in sts:
            statuses.append(GDCA_OK if st.info == 0 else (GDCA_ENOTPD if st.info > 0 else GDCA_ENOCONV))
        for st, s in zip(sts, statuses):
            if s == rc:
                info = st.info
                break
        try:
            self.check(rc, info)
        except Exception as e:
            e.results = results
            e.statuses = statuses
            raise

    def run_multi(self, Zf: np.ndarray, q: int, settings, theta: float, apc: bool = True):
        """gdca_run_multi.  Zf: int8 (N, M), Fortran-contiguous; settings: (pseudocount, score[, apc]) per member (score
        SCORE_FROB | SCORE_DI), one theta for all.  Returns [(S[N,N], stats dict)] in the order of settings, each bit for bit
        what run() gives for that setting."""
        N, M = Zf.shape
        prm, K = _multi_params(settings, theta, apc)
        S = np.empty((max(K, 1), N, N), dtype=np.float64)  # block k = S[k] read as column-major: S[k].T
        sts = (Stats * max(K, 1))()
        rc = self.lib.gdca_run_multi(self.h, _p(Zf), N, M, int(q), prm, K, _p(S), sts)
        results = [(np.asfortranarray(S[k].T), sts[k].as_dict()) for k in range(K)]
        self._check_multi(rc, sts[:K], results)
        return results

    def run_multi_dev(self, Z_ptr: int, N: int, M: int, q: int, settings, theta: float, S_ptr: int, apc: bool = True):
        """Device-pointer form: S_ptr holds K consecutive N x N column-major matrices.  Returns the stats dicts."""
        prm, K = _multi_params(settings, theta, apc)
        sts = (Stats * max(K, 1))()
        rc = self.lib.gdca_run_multi_dev(self.h, C.c_void_p(Z_ptr), int(N), int(M), int(q), prm, K, C.c_void_p(S_ptr), sts)
        results = [sts[k].as_dict() for k in range(K)]
        self._check_multi(rc, sts[:K], results)
        return results

    def run_ranked_multi_ptr(self, Z_ptr: int, N: int, M: int, q: int, settings, theta: float, min_separation: int, apc: bool = True):
        """gdca_run_ranked_multi on a HOST matrix given by address.  Returns [(i, j, score, stats)] in the order of settings, each
        what run_ranked_ptr() gives for that setting."""
        prm, K = _multi_params(settings, theta, apc)
        n = max(int(self.lib.gdca_ranking_length(int(N), int(min_separation))), 0)
        ii = np.empty((max(K, 1), n), dtype=np.int32)
        jj = np.empty((max(K, 1), n), dtype=np.int32)
        sc = np.empty((max(K, 1), n), dtype=np.float64)
        sts = (Stats * max(K, 1))()
        rc = self.lib.gdca_run_ranked_multi(self.h, C.c_void_p(Z_ptr), int(N), int(M), int(q), prm, K, int(min_separation), _p(ii), _p(jj),
                                            _p(sc), sts)
        results = [(ii[k], jj[k], sc[k], sts[k].as_dict()) for k in range(K)]
        self._check_multi(rc, sts[:K], results)
        return results

    def run_ranked_async_ptr(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, score: int, min_separation: int,
                             apc: bool = True):
        """First half of gdca_run_ranked: upload + enqueue, no waiting for the GPU; pair with run_ranked_collect()."""
        prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
        self.check(self.lib.gdca_run_ranked_async(self.h, C.c_void_p(Z_ptr), int(N), int(M), int(q), C.byref(prm), int(min_separation)))
        self._ranked = (int(N), int(min_separation))

    def run_ranked_collect(self):
        """Second half: (i, j, score, stats) of the run enqueued by run_ranked_async_ptr."""
        N, sep = getattr(self, "_ranked", (1, 1))
        n = max(int(self.lib.gdca_ranking_length(N, sep)), 0)
        ii = np.empty(n, dtype=np.int32)
        jj = np.empty(n, dtype=np.int32)
        sc = np.empty(n, dtype=np.float64)
        st = Stats()
        rc = self.lib.gdca_run_ranked_collect(self.h, _p(ii), _p(jj), _p(sc), C.byref(st))
        self.check(rc, st.info)
        return ii, jj, sc, st.as_dict()

    def ranking_dev(self, S_ptr: int, N: int, min_separation: int):
        """compute_ranking of a score matrix in HBM (device pointer), sorted on the device: (i, j, score) host arrays."""
        n = max(int(self.lib.gdca_ranking_length(int(N), int(min_separation))), 0)
        ii = np.empty(n, dtype=np.int32)
        jj = np.empty(n, dtype=np.int32)
        sc = np.empty(n, dtype=np.float64)
        self.check(self.lib.gdca_ranking_dev(self.h, C.c_void_p(S_ptr), int(N), int(min_separation), _p(ii), _p(jj), _p(sc)))
        return ii, jj, sc

    def run_dev(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, score: int,
                S_ptr: int, apc: bool = True):
        """Device-pointer form (Z and S resident in HBM).  Returns the stats dict."""
        prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
        st = Stats()
        rc = self.lib.gdca_run_dev(self.h, C.c_void_p(Z_ptr), N, M, int(q), C.byref(prm), C.c_void_p(S_ptr),
                                   C.byref(st))
        self.check(rc, st.info)
        return st.as_dict()


    def run_dev_async(self, Z_ptr: int, N: int, M: int, q: int, pseudocount: float, theta: float, score: int,
                      S_ptr: int, apc: bool = True):
        """Enqueue only (no host synchronisation); pair with collect()."""
        prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
        self.check(self.lib.gdca_run_dev_async(self.h, C.c_void_p(Z_ptr), N, M, int(q), C.byref(prm),
                                               C.c_void_p(S_ptr)))

    def collect(self):
        st = Stats()
        rc = self.lib.gdca_run_collect(self.h, C.byref(st))
        self.check(rc, st.info)
        return st.as_dict()


def run_dev_phased(ctxs, Z_ptrs, Ns, Ms, qs, pseudocount: float, theta: float, score: int, S_ptrs, apc: bool = True):
    """K families batched by phase on one GPU (gdca_run_dev_phased): K front ends, K inverses back to back, K score
    stages.  Enqueues only; collect() every context afterwards."""
    K = len(ctxs)
    assert K >= 1 and len(Z_ptrs) == len(Ns) == len(Ms) == len(qs) == len(S_ptrs) == K
    prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
    hs = (_ctx * K)(*[c.h for c in ctxs])
    zp = (C.c_void_p * K)(*[C.c_void_p(int(z)) for z in Z_ptrs])
    sp = (C.c_void_p * K)(*[C.c_void_p(int(x)) for x in S_ptrs])
    i32 = lambda v: (C.c_int32 * K)(*[int(x) for x in v])  # noqa: E731
    # (the library copies a failing member's message to the leader: ctxs[0]'s last_error names the member)
    ctxs[0].check(ctxs[0].lib.gdca_run_dev_phased(hs, K, zp, i32(Ns), i32(Ms), i32(qs), C.byref(prm), sp))


def run_ranked_phased_async(ctxs, Z_ptrs, Ns, Ms, qs, pseudocount: float, theta: float, score: int, min_separation: int, apc: bool = True):
    """K families (HOST matrices given by address) through gdca_run_ranked_phased_async: uploads, the phase-batched hot path with
    the small inverses merged, every member's ranking; nothing waited for.  run_ranked_collect() each context afterwards."""
    K = len(ctxs)
    assert K >= 1 and len(Z_ptrs) == len(Ns) == len(Ms) == len(qs) == K
    prm = Params(float(pseudocount), float(theta), int(score), 1 if apc else 0)
    hs = (_ctx * K)(*[c.h for c in ctxs])
    zp = (C.c_void_p * K)(*[C.c_void_p(int(z)) for z in Z_ptrs])
    i32 = lambda v: (C.c_int32 * K)(*[int(x) for x in v])  # noqa: E731
    ctxs[0].check(ctxs[0].lib.gdca_run_ranked_phased_async(hs, K, zp, i32(Ns), i32(Ms), i32(qs), C.byref(prm), int(min_separation)))
    for c, n in zip(ctxs, Ns):
        c._ranked = (int(n), int(min_separation))


def spd_inverse_batch_dev(ctxs, A_ptrs, ns):
    """K independent SPD inverses in place on device matrices (gdca_spd_inverse_batch_dev): the small ones share merged launches
    of the sweep kernel.  Returns the list of info values; raises PosDefException(info of the first failing member)."""
    K = len(ctxs)
    assert K >= 1 and len(A_ptrs) == len(ns) == K
    hs = (_ctx * K)(*[c.h for c in ctxs])
    ap = (C.c_void_p * K)(*[C.c_void_p(int(a)) for a in A_ptrs])
    nn = (C.c_int32 * K)(*[int(x) for x in ns])
    info = (C.c_int32 * K)()
    rc = ctxs[0].lib.gdca_spd_inverse_batch_dev(hs, K, ap, nn, info)
    ctxs[0].check(rc, next((int(i) for i in info if i), 0))
    return [int(i) for i in info]


class DeviceBuffer:
    """An owned HBM allocation (gdca_dbuf): what a host language without a GPU array type keeps the
    intermediates of the statement-by-statement pipeline in.  `.ptr` is the device pointer the `_dev`
    operators take."""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.gdca_dbuf_alloc(ctx.h, int(nbytes), C.byref(h)))
        self.h = h
        self.nbytes = int(ctx.lib.gdca_dbuf_bytes(h))
        self.ptr = int(ctx.lib.gdca_dbuf_ptr(h) or 0)

    @classmethod
    def from_array(cls, ctx: Context, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a) if not (a.flags.c_contiguous or a.flags.f_contiguous) else a
        b = cls(ctx, a.nbytes)
        b.upload(a)
        return b

    def upload(self, a: np.ndarray, offset: int = 0):
        assert a.flags.c_contiguous or a.flags.f_contiguous
        self.ctx.check(self.ctx.lib.gdca_dbuf_upload(self.ctx.h, self.h, int(offset), _p(a), a.nbytes))

    def download(self, shape, dtype=np.float64, order="F", offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype, order=order)
        self.ctx.check(self.ctx.lib.gdca_dbuf_download(self.ctx.h, self.h, int(offset), _p(out), out.nbytes))
        return out

    def copy_from(self, src: "DeviceBuffer", nbytes: int | None = None) -> "DeviceBuffer":
        """The first nbytes (default: all of src) of another buffer into this one, device to device, on the context's stream
        (gdca_dbuf_copy): ordered with every call on the context, nothing crosses to the host."""
        self.ctx.check(self.ctx.lib.gdca_dbuf_copy(self.ctx.h, self.h, src.h, int(src.nbytes if nbytes is None else nbytes)))
        return self

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.gdca_dbuf_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_default_ctx = None


def default_context() -> Context:
    """Process-wide context on the device named by LOCAL_RANK (one process per GPU), else 0."""
    global _default_ctx
    if _default_ctx is None:
        dev = int(os.environ.get("GDCA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        ndev = load().gdca_device_count()
        if ndev <= 0:
            raise GdcaError("no HIP device visible: the gDCA hot path has no CPU fallback")
        ids = visible_devices(ndev)
        _default_ctx = Context(ids[dev % len(ids)])
    return _default_ctx


def visible_devices(ndev: int):
    """GDCA_VISIBLE_DEVICES=0,2,5: the HIP devices this process may use, in that order; unset = all.
    Same rule as gdca_cli --batch: ids outside 0..ndev-1 and repeats are an error."""
    env = os.environ.get("GDCA_VISIBLE_DEVICES", "")
    if not env:
        return list(range(ndev))
    ids = []
    for tok in env.split(","):
        if not tok.strip().isdigit() or int(tok) >= ndev or int(tok) in ids:
            raise ArgumentError(f"invalid GDCA_VISIBLE_DEVICES entry '{tok}' ({ndev} HIP device(s) present)")
        ids.append(int(tok))
    return ids
