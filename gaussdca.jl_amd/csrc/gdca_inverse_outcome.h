// What happens after an SPD inverse has run, and how a call that looked at the device scalars ends: the recovery ladder's
// decisions -- another attempt, the measurement of ||X||_1, the Newton-Schulz step, the Cholesky fallback -- and the verdict, as pure
// functions of plain values.  gdca_api.hip walks the ladder with them (inverse_ladder) and holds no rule of its own; plain C++ without
// a HIP include, so that a host test (tests/test_inverse_outcome_cpu.py compiles this header alone) checks the very same code.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gdca.h"

// ---- the names of the values the kernels leave in gdca_dev_scalars ---------------------------------------------------------------
// bits of bad_symbol: what a kernel found wrong with the caller's data (it goes on with a harmless value in its place)
enum : int {
    GDCA_BAD_ALIGNMENT = 1,   // a byte of Z is outside 1..q (k_bitplane_pack, k_pi_keep)
    GDCA_BAD_WEIGHT = 2,      // a caller-given weight is outside [0, 1] (k_fix_weights)
    GDCA_BAD_SEQUENCE = 4,    // a byte of the scored sequences is outside 1..q (k_energy_pack)
    GDCA_BAD_INDEX = 8,       // an index of gdca_concat_pairs is outside its pool (k_ipa.hip)
    GDCA_BAD_MUTANT = 16,     // a record of gdca_double_mutants is out of range (k_epi_list)
    GDCA_BAD_SLOTS = 32,      // a column of slot0 is no permutation of 0 .. R - 1 (k_temper_init)
};
// info: 0, the 1-based index of the first non-positive pivot, or -- the sweep kernel's watchdog (k_inverse.hip, spin_until) ended the
// launch: a dependency wait ran out of time, nothing is known about the matrix --
enum : int { GDCA_INFO_WATCHDOG = INT32_MIN };

// ---- the ladder -------------------------------------------------------------------------------------------------------------------
// The two callers.  A fused run (gdca_run_collect) screens with the a-priori bound on cond(C) before it measures anything, and a flag in
// bad_symbol ends its ladder: the matrix came from data a kernel has already rejected.  An operator-level inverse (gdca_spd_inverse_dev,
// gdca_spd_inverse_batch_dev) has the caller's matrix at hand, measures both norms whenever refinement is not switched off, and its
// retry and step do not look at bad_symbol (begin() has cleared it and none of its kernels raises a flag).
enum gdca_inverse_form { GDCA_FORM_RUN = 0, GDCA_FORM_OPERATOR = 1 };

// everything the decisions read: the scalars as last fetched, the context's switches, what the record of the run says
struct gdca_inverse_state {
    int form;                                      // gdca_inverse_form
    int info, bad_symbol;                          // gdca_dev_scalars
    double inv_norm1, mat_norm1, ns_resid, pi_max;
    double pc;                                     // the run's pseudocount, N and q (the a-priori bound; an operator leaves them 0)
    int N, q;
    int refine, cholesky;                          // gdca_tuning
    double refine_cond;
    int attempt, retries;                          // attempts the inverse has had beyond the first, and how many it may have
};

// The screen of the fused path costs ordinary families nothing: the covariance with pseudocount pc is that of a MIXTURE -- weight 1 - pc
// on the reweighted alignment, weight pc on independent uniform columns -- so  C >= pc Cov_uniform  in the positive-definite order, and
// Cov_uniform = blockdiag(I / q - 1 1^T / q^2) (q - 1 states a column) has smallest eigenvalue 1 / q^2:
//       lambda_min(C) >= pc / q^2,     cond_2(C) <= ||C||_1 q^2 / pc
// (attained on every alignment tried: a column without gaps makes the bound sharp).  For ||C||_1 two figures: 2 N pi_max, which the
// single-site frequencies give away (k_pi_finalize), and the measured norm (64 .. 94 on the reference's `large` data) where the first
// is not enough -- k_cov_norm1 decides that on the device with this very formula, before the sweep overwrites C.  At the
// pseudocounts gDCA is used with the bound is 1e4 .. 1e5 and the run pays nothing; beyond the threshold the collect measures ||X||_1
// (one pass over the lower triangle) and decides on kappa_1 = ||C||_1 ||X||_1 like the operator-level entry.  +inf where there is no
// bound (pc = 0).
static inline double gdca_cond_bound(double mat_norm1, double pi_max, double pc, int q, int N)
{
    const double c1 = mat_norm1 > 0.0 ? mat_norm1 : 2.0 * (double)N * pi_max;
    if (!(c1 > 0.0) || !(pc > 0.0)) return HUGE_VAL;
    return c1 * (double)q * (double)q / pc;
}

// true where the pseudocount alone bounds cond(C) below the refinement threshold whatever the alignment (pi_max <= (1 - pc) + pc / q):
// then the first build of a covariance (tally_stage, gdca_run_multi) does not even launch k_cov_norm1
static inline bool gdca_norm1_settled(int N, int q, double pc, int refine, double refine_cond)
{
    const double pi_cap = (1.0 - pc) + pc / (double)q;
    return pc > 0.0 && 2.0 * (double)N * pi_cap * (double)q * (double)q / pc <= refine_cond && refine != 1;
}

// The watchdog ended the launch (in practice a launch that did not get all its workgroups back after the driver had taken the device's
// queues off the hardware).  Nothing is wrong with the matrix: it is built again -- the sweep works in place -- and the inverse runs
// again as a launch of its own.  A launch that fails option SWEEP_RETRIES times in a row (default 2) is reported as GDCA_EHIP.
static inline bool gdca_retry_due(const gdca_inverse_state &s)
{
    if (s.info != GDCA_INFO_WATCHDOG || s.attempt >= s.retries) return false;
    return s.form == GDCA_FORM_OPERATOR || !s.bad_symbol;
}

// must ||X||_1 of the inverse be measured (an operator: ||C||_1 of the caller's matrix with it)?  A run asks the a-priori bound first.
static inline bool gdca_norm_due(const gdca_inverse_state &s)
{
    if (s.refine == 0) return false;
    if (s.form == GDCA_FORM_OPERATOR) return true;
    if (s.info != 0 || s.bad_symbol) return false;
    return s.refine == 1 || gdca_cond_bound(s.mat_norm1, s.pi_max, s.pc, s.q, s.N) > s.refine_cond;
}

// The inverse looks ill-conditioned: the block sweep's error grows like cond^2, so it gets one Newton-Schulz step against the matrix.
static inline bool gdca_wants_refinement(const gdca_inverse_state &s)
{
    if (s.info != 0 || s.refine == 0) return false;
    if (s.form == GDCA_FORM_RUN && s.bad_symbol) return false;
    if (s.refine == 1) return true;
    if (!(s.inv_norm1 > 0.0)) return false;  // not measured: the a-priori bound on cond(C) was below the threshold
    // kappa_1 = ||C||_1 ||X||_1 (||C||_1: the covariance build's, or the caller's matrix at the operator-level entry)
    return s.inv_norm1 * (s.mat_norm1 > 0.0 ? s.mat_norm1 : 1.0) > s.refine_cond;
}

// gdca_stats.refined once the step has run.  It squares I - X0 C: with that residual at one or beyond (cond(C) past ~1e10: the sweep's
// own error is of order one there) it cannot have converged, and the caller is told so instead of being handed the result as if it
// were refined.  (The codes: 0 no step, 1 refined, -1 the step could not converge, 2 the Cholesky fallback's inverse.)
static inline int gdca_refined_after_step(const gdca_inverse_state &s)
{
    return s.ns_resid < 1.0 ? 1 : -1;
}

// The reference's own factorisation as the last resort (option CHOLESKY: 0 never, 1 where the sweep gave up, 2 always [tests]):
// the sweep reported a non-positive pivot -- beyond cond ~1e10 that can be its own rounding, LAPACK's dpotrf still factors such
// matrices -- or its Newton-Schulz step could not converge.  `s`: the scalars as fetched after the sweep / the step.
static inline bool gdca_wants_cholesky(const gdca_inverse_state &s, int refined)
{
    if (s.cholesky == 0 || s.bad_symbol || s.info == GDCA_INFO_WATCHDOG) return false;
    return s.cholesky == 2 || s.info > 0 || refined < 0;
}

// ---- the verdict ------------------------------------------------------------------------------------------------------------------
#define GDCA_TEXT_BAD_SEQUENCE "sequences hold a symbol outside 1..q"
#define GDCA_TEXT_BAD_MUTANT "a double-mutant record is out of range"
#define GDCA_TEXT_BAD_ALIGNMENT "alignment holds a symbol outside 1..q"
#define GDCA_TEXT_WATCHDOG "SPD inverse aborted: a dependency wait inside the sweep kernel timed out"
#define GDCA_TEXT_COV_NOT_PD "covariance matrix is not positive definite"
#define GDCA_TEXT_MATRIX_NOT_PD "matrix is not positive definite; Cholesky factorization failed"
#define GDCA_TEXT_DI_NOCONV "eigenvalue iteration of a DI block did not converge"

// which kind of call is ending: it says which of the scalars the call has a stake in
enum gdca_call_kind {
    GDCA_ENDS_RUN = 0,       // a fused run's collect: every flag, the inverse's info, the DI iteration
    GDCA_ENDS_INVERSE = 1,   // an operator-level inverse: info alone
    GDCA_ENDS_READOUT = 2,   // a read-out operator (energies, pair energies, scans): the flags of its sequences and records
    GDCA_ENDS_FRONT = 3,     // a front-end operator (neighbour counts, weights, frequencies): the flags of its alignment
};

struct gdca_verdict {
    gdca_status status;
    const char *text;  // what gdca_last_error returns (nullptr with GDCA_OK)
};

// In the order a caller can act on: the scored sequences, the listed records, any other flag (told as the alignment's; a read-out has
// no alignment and tells it as its sequences'), the watchdog, the matrix, the DI iteration.
static inline gdca_verdict gdca_verdict_of(int kind, int bad_symbol, int info, int di_noconv)
{
    const bool run = kind == GDCA_ENDS_RUN, readout = kind == GDCA_ENDS_READOUT;
    if (run && (bad_symbol & GDCA_BAD_SEQUENCE)) return {GDCA_EINVAL, GDCA_TEXT_BAD_SEQUENCE};
    if ((run || readout) && (bad_symbol & GDCA_BAD_MUTANT)) return {GDCA_EINVAL, GDCA_TEXT_BAD_MUTANT};
    if (kind != GDCA_ENDS_INVERSE && bad_symbol) return {GDCA_EINVAL, readout ? GDCA_TEXT_BAD_SEQUENCE : GDCA_TEXT_BAD_ALIGNMENT};
    if (run || kind == GDCA_ENDS_INVERSE) {
        if (info == GDCA_INFO_WATCHDOG) return {GDCA_EHIP, GDCA_TEXT_WATCHDOG};
        if (info != 0) return {GDCA_ENOTPD, run ? GDCA_TEXT_COV_NOT_PD : GDCA_TEXT_MATRIX_NOT_PD};
    }
    if (run && di_noconv != 0) return {GDCA_ENOCONV, GDCA_TEXT_DI_NOCONV};
    return {GDCA_OK, nullptr};
}

// gdca_spd_inverse_batch_dev reports its worst member: a launch the watchdog ended wherever it stands, else the first matrix that is
// not positive definite
static inline gdca_verdict gdca_worse_verdict(const gdca_verdict &so_far, const gdca_verdict &member)
{
    return member.status == GDCA_EHIP || so_far.status == GDCA_OK ? member : so_far;
}
