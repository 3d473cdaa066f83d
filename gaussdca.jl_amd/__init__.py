"""gaussdca.jl_amd -- MI355X (gfx950) Gaussian-DCA hot path behind GaussDCA.jl's interface.

``gDCA`` / ``printrank`` mirror the reference module's exports (src/GaussDCA.jl:3); the
DCAUtils-named operators are in :mod:`dcautils`.  All hot-path arithmetic runs in the HIP
library ``libgdca.so`` (C-ABI: include/gdca.h); importing this package never falls back to a
CPU implementation -- calling any operator without the built library or without a GPU raises.
"""
from ._lib import run_dev_phased, run_ranked_phased_async, spd_inverse_batch_dev  # noqa: F401
from ._lib import (ArgumentError, Context, ConvergenceError, DeviceBuffer, GdcaError, PosDefException,  # noqa: F401
                   default_context, load)
from .dcautils import double_mutant_energies, double_mutant_scan  # noqa: F401
from .gdca import gDCA_double_mutant_scan, gDCA_double_mutants  # noqa: F401
from .dcautils import greedy_walk  # noqa: F401
from .gdca import gDCA_greedy_walk  # noqa: F401
from .dcautils import sample  # noqa: F401
from .dcautils import sample_tempered  # noqa: F401
from .gdca import gDCA_sample  # noqa: F401
from .gdca import gDCA_sample_tempered  # noqa: F401
from .dcautils import bm_learn, potts_from_gaussian, potts_independent  # noqa: F401
from .gdca import gDCA_bm  # noqa: F401
from .dcautils import plm_conditionals, plm_learn, plm_tallies  # noqa: F401
from .gdca import gDCA_plm  # noqa: F401
from .dcautils import log_partition, potts_loglik  # noqa: F401
from .dcautils import (add_pseudocount, assign_blocks, compute_C, compute_DI_gauss, compute_FN, compute_ranking,  # noqa: F401
                       compute_theta, compute_weighted_frequencies, compute_weights, correct_APC,
                       inv_cholesky, logodds_information, mutation_scan, neighbour_counts, pair_energies, pair_energies_blocked, pair_identity_sum,
                       pair_logodds, pair_logodds_blocked, printrank,
                       read_fasta_alignment, remove_duplicate_sequences, sequence_energies, sequence_loglik, species_blocks, Ranking)
from .gdca import (check_arguments, gDCA, gDCA_energies, gDCA_loglik, gDCA_multi, gDCA_mutation_scan, gDCA_pair_energies,  # noqa: F401
                   gDCA_pair_logodds, gDCA_partner_ipa, gDCA_partner_logodds, gDCA_partner_match)

__all__ = ["gDCA", "printrank"]
