/* gdca.h -- C-ABI of libgdca.so: the MI355X (gfx950) Gaussian-DCA hot path.
 *
 * This is the drop-in boundary for the one path of carlobaldassi/GaussDCA.jl that this
 * project accelerates: everything between src/GaussDCA.jl:28 and :42 of the reference
 *
 *     Pi_true, Pij_true, Meff, _ = compute_weighted_frequencies(Z, q, theta)   (:28)
 *     Pi, Pij = add_pseudocount(Pi_true, Pij_true, Float64(pseudocount), q)     (:30)
 *     C  = compute_C(Pi, Pij)                                                   (:32, :76)
 *     mJ = inv(cholesky(C))                                                     (:34)
 *     S  = score == :DI ? compute_DI_gauss(mJ, C, q) : compute_FN(mJ, q)        (:36-40)
 *     S  = correct_APC(S)                                                       (:42, :78-86)
 *
 * The reference is Julia; it would bind these entry points with `ccall((:sym, libgdca), ...)`
 * (the stub a maintainer would add is in INTEGRATION.md).  Plain pointers and sizes only: no
 * C++ types, no exceptions, no Julia/Python/torch types cross this ABI.
 *
 * Conventions
 *   - Matrices are COLUMN-MAJOR (Julia native), so Julia arrays are passed without copies.
 *   - Z is the reference's `Z::Matrix{Int8}`, N x M column-major: sequence k is the N
 *     contiguous bytes Z[k*N .. k*N+N-1], symbols 1..q, q <= 31 (src/GaussDCA.jl:24-26).
 *   - s = q - 1 (state q, the gap, has no row/column); n = N * s.
 *   - "host" pointers are ordinary host memory owned by the caller; "_dev" entry points take
 *     device (HBM) pointers owned by the caller.  The library never returns memory it
 *     allocated except the opaque gdca_ctx.
 *   - Every function returns a gdca_status; it never aborts and never throws.
 *   - A gdca_ctx owns one HIP device, one stream and a grow-only device workspace.  A ctx is
 *     used by one host thread at a time; different ctxs are independent (this is the
 *     multi-GPU model: one ctx per GPU, no collectives).
 *   - There is NO CPU fallback: without a usable HIP device gdca_ctx_create fails with
 *     GDCA_EHIP and nothing else can be called.
 */
#ifndef GDCA_H
#define GDCA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest covariance the entry points accept: n = N (q-1) <= GDCA_MAX_N (a 60 000 x 60 000 f64 matrix is 28.8 GB of the
 * 288 GB of HBM; the sweep kernel's item tables are 32-bit).  Exercised up to n = 48 000. */
#define GDCA_MAX_N 60000

#define GDCA_VERSION_MAJOR 0
#define GDCA_VERSION_MINOR 6

typedef enum gdca_status {
    GDCA_OK = 0,
    GDCA_EINVAL = 1, /* bad argument: mirrors ArgumentError (src/GaussDCA.jl:50-62) and q >= 32 (:26) */
    GDCA_ENOTPD = 2, /* covariance not positive definite: mirrors PosDefException(info) from :34 */
    GDCA_EHIP = 3,   /* HIP runtime error; see gdca_last_error() */
    GDCA_ENOMEM = 4, /* device or host allocation failed */
    GDCA_ENOCONV = 5 /* eigenvalue iteration inside compute_DI_gauss did not converge: mirrors the LAPACKException
                        eigen()/eigvals() would raise inside DCAUtils (call site :37); stats.info = -(pairs affected) */
} gdca_status;

enum { GDCA_SCORE_FROB = 0, GDCA_SCORE_DI = 1 }; /* score = :frob | :DI (src/GaussDCA.jl:14) */

typedef struct gdca_ctx gdca_ctx;
typedef struct gdca_dbuf gdca_dbuf; /* an owned HBM allocation (see "device buffers" below) */

/* Keyword arguments of gDCA() that reach the hot path (src/GaussDCA.jl:10-15). */
typedef struct gdca_params {
    double pseudocount; /* 0 <= pc <= 1            (default 0.8, :11)                       */
    double theta;       /* 0 <= theta <= 1, or any negative value for theta = :auto (:12)   */
    int32_t score;      /* GDCA_SCORE_FROB | GDCA_SCORE_DI (:14)                            */
    int32_t apc;        /* 1: apply correct_APC (what gDCA does, :42); 0: raw scores        */
} gdca_params;

/* What DCAUtils prints (theta, threshold, Meff) plus device timings of the last run. */
typedef struct gdca_stats {
    double theta;               /* theta used (the estimate when theta = :auto)             */
    double Meff;                /* effective number of sequences                            */
    uint64_t pair_identity_sum; /* sum_{k<l} #{i: Z[i,k]==Z[i,l]} (0 unless theta = :auto)  */
    int32_t thresh;             /* floor(theta * N)                                         */
    int32_t info;               /* 0; k>0: leading minor k of C not positive definite;
                                   k<0: -k site pairs whose DI eigenvalue iteration failed  */
    int32_t N, M, q, n, n_pad;  /* n = N(q-1); n_pad = n rounded up to the tile size        */
    int32_t update_launches;    /* launches of the dominant kernel this run accounts for (a merged launch: its first member) */
    int32_t inverse_batch;      /* families that shared this run's SPD-inverse launch (gdca_run_dev_phased merges the small ones;
                                   1 = a launch of its own).  ms_inverse and ms_inverse_update are the launch's time divided by it */
    int32_t refined;            /* 1: the covariance is ill-conditioned (kappa_1 = matrix_norm1 * inverse_norm1 beyond REFINE_COND) and the inverse got a Newton-Schulz
                                   step, the scores were computed again from it (the ms_* are those of the first pass);
                                   -1: the step was taken but cannot have converged (residual |I - X C| >= 1: cond(C) beyond ~1e10,
                                   where the sweep's own error is of order one) and option CHOLESKY is 0 -- the scores are not
                                   to be trusted;
                                   2: the sweep gave up (a non-positive pivot of its own, or the step above could not converge) and
                                   the inverse was computed again by blocked Cholesky (dpotrf + dpotri, as the reference does);
                                   `info` and the scores are those of that factorisation */
    /* device time, milliseconds: between two boundaries of the run's timeline, both marked by one clock -- HIP events on the ctx
       stream, or, for the members of a phase batch issued as batched grids, 100 MHz device time stamps written by kernels of the
       batch (a launch of its own is bracketed by events there too).  0: the run did not mark that stage, or timing is off */
    double ms_total;            /* Z in HBM -> S in HBM                                     */
    double ms_theta;            /* column histograms + theta                                */
    double ms_weights;          /* bit-plane pack + all-pairs Hamming + W, Meff             */
    double ms_covariance;       /* Pi + pair tallies + pseudocount + covariance build       */
    double ms_inverse;          /* SPD inverse, whole stage                                 */
    double ms_inverse_update;   /* sum over launches of the dominant kernel                 */
    double ms_score;            /* FN or DI, + APC                                          */
    double inverse_flops;       /* n^3/3+n^2/2+n/6 + 2n^3/3+n^2/2+5n/6 (dpotrf+dpotri)      */
    double update_flops;        /* flops executed by all launches of the dominant kernel    */
    double sweep_ghz;           /* shader clock during the SPD-inverse kernel, measured by the kernel itself
                                   (s_memtime cycles / 100 MHz wall-clock ticks, summed over its workgroups); 0 if no inverse ran */
    double inverse_norm1;       /* ||inv(C)||_1 as the sweep left it, measured (one pass over the inverse) only where cond_bound is
                                   beyond REFINE_COND: the decision on a refinement is kappa_1 = matrix_norm1 * inverse_norm1 >
                                   REFINE_COND.  0: not measured (the bound settled it, or option REFINE=0) */
    double matrix_norm1;        /* ||C||_1 of the covariance (src/GaussDCA.jl:32), measured (one pass over C before the sweep overwrites
                                   it) only where the bound that costs nothing, ||C||_1 <= 2 N max_i Pi(i), leaves cond_bound beyond
                                   REFINE_COND: 64 .. 94 on the reference's test/data/large.fasta.gz, not "of order one".  0: not
                                   measured (the cheap bound settled it, or option REFINE=0) */
    double cond_bound;          /* a-priori bound of cond_2(C): ||C||_1 q^2 / pseudocount, with matrix_norm1 where it was measured
                                   and 2 N max Pi otherwise.  The covariance with pseudocount pc is that of a mixture with weight pc
                                   on independent uniform columns, hence lambda_min(C) >= pc / q^2 (sharp whenever some column has
                                   no gap).  Every run whose bound is below REFINE_COND is KNOWN to be well enough conditioned
                                   for the sweep and pays nothing for the screen; +inf at pseudocount 0; 0 with option REFINE=0 */
    /* Fields are only ever added at the END, and every addition bumps GDCA_VERSION_MINOR (0.5: the five fields from
     * matrix_norm1 on; 0.6: sweep_retries).  The LIBRARY fills sizeof(gdca_stats) as IT was built: a binding built against a newer header than
     * the library reads a valid prefix (the rest stays as the caller initialised it), but a binding built against an OLDER,
     * shorter struct would be overrun -- so a binding compares gdca_stats_bytes() with its own struct size (and
     * gdca_version() with the minor it was written for) once at load time and refuses to run on a mismatch, as the Python
     * and Julia bindings of this repository do. */
    double ms_fn;               /* the FN kernel alone (HBM-bound: one pass over the lower block triangle of the inverse,
                                   8 n (n - s) / 2 bytes); 0 for the DI score and for a run refined at collect time */
    double ms_pair_tally;       /* the pair-tally kernel alone, with its pseudocount + covariance epilogue (its one
                                   compulsory HBM write: 8 n^2 bytes); 0 with option REFINE=0                      */
    int32_t sweep_retries;      /* 0.6: times this run's SPD inverse was run AGAIN because the sweep kernel's watchdog had ended
                                   its launch (normally 0; see "Contexts and the device's queues" below).  The result is that
                                   of the last attempt; ms_inverse, ms_inverse_update, ms_score and ms_fn are the last attempt's
                                   (its score stage ran alone: no share of a batch), and ms_total runs to the end of the last attempt */
    int32_t reserved0;          /* (keeps the struct a multiple of 8 bytes; 0) */
} gdca_stats;

/* ---- library / context ---------------------------------------------------------------- */
int32_t gdca_version(void); /* major*1000 + minor */
/* sizeof(gdca_stats) / sizeof(gdca_params) as this build of the library writes / reads them (see the note at the end of gdca_stats) */
int32_t gdca_stats_bytes(void);
int32_t gdca_params_bytes(void);
int32_t gdca_device_count(void);

/* Contexts and the device's queues.  A context owns a stream, and a stream's hardware queue comes into being with its first command;
 * the driver maps a new queue by taking EVERY queue of the device off the hardware and back -- the waves of all running kernels are
 * saved and restored (~1.7 ms).  A persistent sweep restored beside the kernels of other queues may not get all its workgroups back
 * and then stands still until its watchdog ends it (round 6; gdca_api.hip, warm_stream; k_inverse.hip, spin_until).  Therefore:
 *   - gdca_ctx_create / _create_peer make the stream's queue at once (a small fill and a synchronisation: ~0.2 ms more per context);
 *   - make the contexts a program needs BEFORE it enqueues work, as the batch driver and bench.py do.  A context on a caller's stream
 *     (gdca_ctx_create_on_stream) is the caller's business: run something on that stream first;
 *   - what a program cannot rule out (another process starting on the GPU, a library of its own that makes a stream) is survived: the
 *     sweep notices that its waves were off the hardware and ends a launch that no longer moves after ~0.1 s instead of seconds, and
 *     gdca_run_collect / gdca_spd_inverse_dev run that inverse again -- up to option SWEEP_RETRIES (default 2) times, reported in
 *     gdca_stats.sweep_retries; the results are those of an undisturbed run: bit for bit for launches of their own and for
 *     members of a merged launch under option MERGE_GROUP=1, equal to rounding for a member of a merged launch with the library's own
 *     grouping (the second attempt is a launch of its own, swept in the pivot groups of that size).  Only an inverse that fails every
 *     attempt is GDCA_EHIP ("a dependency wait inside the sweep kernel timed out"). */
gdca_status gdca_ctx_create(int32_t device_id, gdca_ctx **out);
/* same, but enqueue on an existing hipStream_t (passed as void*); NULL = the null stream */
gdca_status gdca_ctx_create_on_stream(int32_t device_id, void *hip_stream, gdca_ctx **out);
/* A further context on the leader's device that forms a PIPELINE with it: runs enqueued on the members
 * execute their SPD-inverse stages one after the other (device-side event chain), so that with
 * gdca_run_dev_async the reweighting/tally stages of the next family overlap the inverse of the current
 * one.  All members of a pipeline are driven by one host thread.  Contexts that run on one GPU at the same time SHOULD be such
 * peers: the SPD inverse is a persistent kernel, and two of them side by side only take turns for the compute units.  Sharing the device
 * WITHOUT a gate is slower, not unsafe: launches of one family each and merged launches (gdca_run_dev_phased) beside another sweep -- two
 * non-peer contexts driven by two threads, two processes -- all finish with the right inverses (tested: INTEGRATION.md, "Sharing a device"). */
gdca_status gdca_ctx_create_peer(gdca_ctx *leader, gdca_ctx **out);
gdca_status gdca_ctx_destroy(gdca_ctx *ctx);
gdca_status gdca_ctx_synchronize(gdca_ctx *ctx);
const char *gdca_last_error(gdca_ctx *ctx); /* valid until the next call on ctx */
/* per-stage device timing (HIP events + one stream sync per run); default on */
gdca_status gdca_ctx_set_timing(gdca_ctx *ctx, int32_t enabled);
/* Tuning switch of THIS context (no process-global state: a context reads the GDCA_* environment variables once, when it is
 * created; afterwards only this call changes them, and two contexts of one process may differ).  key = the variable's name with
 * or without the GDCA_ prefix, any case; value = what the variable would hold.  Schedule of the SPD inverse: GROUP (1..4, -1 = the
 * measured rule), RAMP, RAGGED, REM_TAIL, PANEL_HALVES, SLAB, RING, MCUS, MCU_SOLO; SWEEP_TIMEOUT_MS (bound of one dependency wait inside
 * the sweep kernel; 0 = scaled with the problem, at least 4 s), SWEEP_RETRIES (0..5: further attempts of an inverse whose launch the watchdog ended), SWEEP_DEBUG, SWEEP_TRACE (file); HAMMING_MODE (auto | full |
 * bound | mfma: which form counts the neighbours -- auto [default] picks per family from sampled tiles; full = exact five-plane distances; bound = the three low planes as a lower bound; mfma = the consensus plane,
 * "differs from the column's most frequent symbol", as a lower bound on the fp4 matrix pipe; either bound's listed pairs are counted exactly: the same integers whatever the form), HAM_CUT (tests, measurements: the word at which the three-plane bound goes from all pairs of a tile to
 * the pairs still below the threshold; 0 = chosen per family from the sampled tiles [default], k >= 1 = word k, beyond the last word = never: the same counts whatever it is), FORCE_FALLBACK (the independent byte-compare Hamming kernel, cf. DCAUTILS_FORCE_FALLBACK in test/runtests.jl:78-86),
 * TALLY_TJ; TALLY_SKIP (1 = the pair tally skips each column's most frequent symbol and recovers that row from the single-site sums
 * [default], 0 = it tallies every sequence: the same bits either way); MERGE (families per merged SPD-inverse launch in gdca_run_dev_phased, 1 = off), MERGE_BLOCKS (largest member, in
 * 128-blocks), MERGE_TILES, MERGE_GROUP, MERGE_MCUS, PHASED_FRONTS (1: the front ends of a phase batch run side by side on the
 * members' streams, 0: one after the other), PHASED_STREAMS (how many of those streams, the first members', they are spread over: default 4), PHASED_GRIDS (the kernels of a phase batch as ONE grid per kernel kind carrying all members of a group: -1 = 1 group for small families, 4 for big ones [default], 1 .. 8 = that many groups side by side, 0 = a launch per member and kernel as PHASED_FRONTS describes); REFINE (auto | 0 | 1: one Newton-Schulz step on an inverse that looks
 * ill-conditioned / never / always) and REFINE_COND (the threshold of auto, default 1e6); CHOLESKY (0 | 1 | 2: the blocked
 * dpotrf + dpotri fallback never / where the sweep gave up [default] / for every inverse); ENERGY_CHUNK (sequences one launch of the energy gather
 * kernel takes, 0 = the rule [default]: the same bits whatever it is); PAIR_CHUNK (sequences of protein A one launch of the pair-energy
 * kernels takes, 0 = the rule [default: a ~256 MB buffer]; a count above the rule's is cut to it: the same bits whatever it is); WALK_TABLE (auto | lds | hbm: where the greedy walk keeps a
 * sequence's table of site potentials -- auto [default]: in LDS where it fits, else in HBM; lds with a table that does not fit makes the
 * walk fail with GDCA_EINVAL; the same bits wherever it is; the Metropolis chains place their table by the same rule and the same option);
 * SAMPLE_CHUNK (proposals one launch of the Metropolis kernel takes, 0 = the rule [default]: 65536; the same bits whatever it is);
 * PLM_CHUNK (sequences a block of the pseudo-likelihood tally adds in one go, 0 = the rule [default]: 512; it FIXES THE ORDER of the tally's
 * sums, so another value gives other bits); PLM_SLAB (sequences whose conditionals are held at a time, rounded up to whole blocks, 0 = the
 * rule [default: a ~256 MB table]; the same bits whatever it is).  The schedule switches change results
 * at rounding level at most (another summation order); REFINE improves an ill-conditioned inverse.  GDCA_EINVAL: unknown key
 * or unusable value. */
gdca_status gdca_ctx_set_option(gdca_ctx *ctx, const char *key, const char *value);

/* ---- fused hot path: replaces src/GaussDCA.jl:28-42 in one call ------------------------ */
/* Z_host: N x M int8 (host).  S_host: N x N f64 column-major (host), caller-owned.
 * Only Z goes in and S + stats come out over PCIe. */
gdca_status gdca_run(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q,
                     const gdca_params *p, double *S_host, gdca_stats *st);
/* Same with Z and S resident in HBM (device pointers). Synchronises the ctx stream before
 * returning so that *st is complete. */
gdca_status gdca_run_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q,
                         const gdca_params *p, double *S_dev, gdca_stats *st);

/* ---- several settings of ONE alignment in one call ----------------------------------------------------------------------
 * The reference's two standard rankings (FN at pseudocount 0.8, DI at 0.2) or a scan of the pseudocount over one family.  p and st
 * have K entries, 1 <= K <= GDCA_MULTI_MAX; every p[k].theta must be the same setting (equal, or all negative = :auto) and every
 * p[k] valid as for gdca_run, else GDCA_EINVAL with nothing run.  Outputs are K consecutive blocks in the order of p: S_* holds K
 * column-major N x N matrices, i_out / j_out / score_out K blocks of gdca_ranking_length(N, min_separation) entries.
 * What does not depend on the setting runs ONCE: theta, the reweighting, Pi and the pair tallies, kept as Pij_true in a grow-only
 * context buffer of n x n f64 (one buffer whatever K: 0.8 GB at n = 10 000, 28.8 GB at GDCA_MAX_N, on top of the covariance).  Then,
 * for every distinct pseudocount in order of first appearance (a "group"), the covariance is built from Pij_true, the DI diagonal
 * blocks where a member asks for DI, and the SPD inverse; each member of the group gets its score, APC and ranking from that
 * inverse.  Every member's output is bit for bit that of gdca_run / gdca_run_ranked with p[k] (K = 1 is that very call).
 * Conditioning is per group: the refinement screen, the Newton-Schulz step, the Cholesky fallback and the sweep's second attempt
 * are those a single run of the group's pseudocount takes (each rebuilds C from Pij_true).  A member that fails (GDCA_ENOTPD, e.g.
 * pc = 0 with a constant column; GDCA_ENOCONV) leaves the others computed: the call returns the status of the first failing member
 * in the order of p, every st[k].info is what a single run would report, and a failing member's outputs are unspecified.
 * GDCA_EHIP, GDCA_ENOMEM and an alignment with a symbol outside 1..q end the whole call.  Synchronous.
 * Stats: theta, Meff, pair_identity_sum, thresh, ms_theta and ms_weights are the shared front end's, the same in every entry.
 * ms_covariance is the pair tally + build for the first group and only the build from Pij_true for the others; refined, info (but
 * a DI member's ENOCONV count), cond_bound, matrix_norm1, inverse_norm1, sweep_retries, sweep_ghz and the ms_inverse* are the
 * group's; ms_score and ms_fn the member's own; ms_total runs from the start of the call to the end of the member's score stage;
 * ms_pair_tally is 0. */
#define GDCA_MULTI_MAX 16
gdca_status gdca_run_multi(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K,
                           double *S_host, gdca_stats *st);
gdca_status gdca_run_multi_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K,
                               double *S_dev, gdca_stats *st);
/* The same with the device ranking of every member (gdca_run_ranked): Z (host) in, K rankings out; no score matrix crosses PCIe. */
gdca_status gdca_run_ranked_multi(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K,
                                  int32_t min_separation, int32_t *i_out, int32_t *j_out, double *score_out, gdca_stats *st);

/* Split form for pipelining independent families over several contexts on one GPU: _async only
 * enqueues (no host synchronisation); gdca_run_collect waits for that run, fills *st and returns the run's
 * status.  One run may be outstanding per ctx (a second _async before the collect is GDCA_EINVAL); the Z and S
 * buffers must stay valid until it is collected. */
gdca_status gdca_run_dev_async(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q,
                               const gdca_params *p, double *S_dev);
gdca_status gdca_run_collect(gdca_ctx *ctx, gdca_stats *st);
/* K independent families batched BY PHASE on one GPU (throughput form of the same path; the reference's only statement on
 * parallelism is "independent families", README.md:92-94): the K front ends (theta, reweighting, tallies, covariance), then
 * the K SPD inverses back to back, then the K score stages, all on the stream of ctxs[0].  The matrix pipes see one
 * uninterrupted stretch of MFMA work per batch instead of K load steps (the clock governor answers every step from the
 * front end's VALU/LDS work to the inverse with a dip that costs ~10 % of an inverse at n = 10 000), and results are bit for
 * bit those of K single runs.  K distinct contexts of one device (each keeps its own workspace: K covariance matrices
 * live at once), none with a run outstanding; arrays of K entries; one parameter set.  Enqueues only: collect every
 * member with gdca_run_collect (any order).  K <= 64. */
gdca_status gdca_run_dev_phased(gdca_ctx *const *ctxs, int32_t K, const int8_t *const *Z_dev, const int32_t *N,
                                const int32_t *M, const int32_t *q, const gdca_params *p, double *const *S_dev);

/* ---- device buffers ---------------------------------------------------------------------- */
/* For callers without a GPU array type of their own (the Julia shim): an owned allocation in the HBM of ctx's
 * device.  gdca_dbuf_ptr() is the plain device pointer the `_dev` entry points take (any other device pointer of
 * the same GPU, e.g. a torch tensor's data_ptr, is as good).  upload/download are synchronous. */
gdca_status gdca_dbuf_alloc(gdca_ctx *ctx, uint64_t bytes, gdca_dbuf **out);
gdca_status gdca_dbuf_free(gdca_dbuf *buf);
void *gdca_dbuf_ptr(const gdca_dbuf *buf);
uint64_t gdca_dbuf_bytes(const gdca_dbuf *buf);
gdca_status gdca_dbuf_upload(gdca_ctx *ctx, gdca_dbuf *buf, uint64_t offset, const void *host, uint64_t bytes);
gdca_status gdca_dbuf_download(gdca_ctx *ctx, const gdca_dbuf *buf, uint64_t offset, void *host, uint64_t bytes);
/* the first `bytes` bytes of src into dst, device to device, enqueued on ctx's stream behind what has been enqueued (not synchronous) */
gdca_status gdca_dbuf_copy(gdca_ctx *ctx, gdca_dbuf *dst, const gdca_dbuf *src, uint64_t bytes);

/* ---- operator level, device-resident: the statements of src/GaussDCA.jl:28-42 one by one with every array in HBM --
 * Same meaning as the host-pointer operators below (which are "upload, call the _dev form, download"); array
 * arguments are device pointers, scalars come back through host pointers.  Dense matrices are n x n column-major
 * with leading dimension n (n = N (q-1)).  A maintainer who keeps the reference's statement-by-statement gDCA()
 * moves only Z in and S out over PCIe:
 *     W, Meff           <- gdca_compute_weights_dev            (compute_weights inside :28)
 *     Pi_true, Pij_true <- gdca_frequencies_dev                (:28)
 *     Pi, Pij           <- gdca_add_pseudocount_dev            (:30; may run in place)
 *     C                 <- gdca_covariance_dev                 (:32, :76; C may alias Pij)
 *     mJ                <- gdca_spd_inverse_dev                (:34; in place)
 *     S                 <- gdca_fn_dev | gdca_di_dev           (:37, :39)
 *     S                 <- gdca_apc_dev                        (:42; in place)                                         */
gdca_status gdca_pair_identity_sum_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, uint64_t *out);
gdca_status gdca_compute_theta_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, double *theta);
gdca_status gdca_neighbour_counts_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t thresh,
                                      int32_t *n_dev);
gdca_status gdca_compute_weights_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, double theta,
                                     double *W_dev, double *Meff, double *theta_used, int32_t *thresh);
gdca_status gdca_frequencies_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q,
                                 const double *W_dev, double Meff, double *Pi_dev, double *Pij_dev);
gdca_status gdca_add_pseudocount_dev(gdca_ctx *ctx, const double *Pi_true_dev, const double *Pij_true_dev, int32_t N,
                                     int32_t q, double pc, double *Pi_dev, double *Pij_dev);
gdca_status gdca_covariance_dev(gdca_ctx *ctx, const double *Pi_dev, const double *Pij_dev, int32_t n, double *C_dev);
gdca_status gdca_spd_inverse_dev(gdca_ctx *ctx, double *A_dev, int32_t n, int32_t *info);
/* K independent inv(cholesky(.)) on one GPU (:34, for K families at once): A_dev[k] (n[k] x n[k], full symmetric, device) is
 * replaced by its inverse; info[k] as gdca_spd_inverse (info may be NULL).  The small members -- up to MERGE_BLOCKS 128-blocks,
 * which leave most of the chip idle when they run alone -- share launches of the sweep kernel, MERGE of them at a time
 * (gdca_ctx_set_option on ctxs[0]); every result is bit for bit that of gdca_spd_inverse_dev.  K <= 64 distinct contexts of
 * one device (a member's workspace is its context's).  Synchronous.  GDCA_ENOTPD if any member is not positive definite.  Like
 * gdca_spd_inverse_dev, a member whose kappa_1 = ||A||_1 ||inv A||_1 is beyond REFINE_COND gets one Newton-Schulz step. */
gdca_status gdca_spd_inverse_batch_dev(gdca_ctx *const *ctxs, int32_t K, double *const *A_dev, const int32_t *n, int32_t *info);
gdca_status gdca_fn_dev(gdca_ctx *ctx, const double *mJ_dev, int32_t N, int32_t q, double *S_dev);
gdca_status gdca_di_dev(gdca_ctx *ctx, const double *mJ_dev, const double *C_dev, int32_t N, int32_t q, double *S_dev);
gdca_status gdca_apc_dev(gdca_ctx *ctx, double *S_dev, int32_t N);

/* ---- energies: scoring sequences under the fitted model ------------------------------------------------------------------
 * The other use of mJ = inv(cholesky(C)) (src/GaussDCA.jl:34): the likelihood of a sequence under the multivariate Gaussian whose
 * covariance :32 builds (the paper's "protein-interaction partners" half: partner matching, filtering, ranking variants).  With the
 * one-hot encoding x of a sequence (x[i*s + a - 1] = 1 for symbol a in 1..s at 0-based site i; symbol q, the gap, leaves the site's
 * block zero) and Pi the single-site frequencies WITH pseudocount (add_pseudocount's first result, :30):
 *     E(x) = 1/2 (x - Pi)' mJ (x - Pi)
 * i.e. minus the log-likelihood up to the model's constant 1/2 log det(2 pi C), which is not part of E: comparisons inside one model
 * never need it.  Comparisons ACROSS models do -- see "log-likelihoods" below (gdca_last_logdet, gdca_run_loglik), which supply it from
 * the pivots of the very inverse the model comes from.  Lower energy = better fit.
 * X is N x K int8 column-major like Z (sequence k = the N bytes X[k*N ..]), K >= 1; E has K entries.  mJ is n x n column-major,
 * leading dimension n, symmetric: only its lower triangle is read.  Every sum is taken in a fixed order in f64 (no floating-point
 * atomics): a sequence's energy is the same bits from run to run, whatever other sequences share the call and wherever it stands
 * among them.  GDCA_EINVAL: K < 1, q outside 2..31, a null pointer -- nothing is run -- or a byte of X outside 1..q (detected on the
 * device; nothing is read out of bounds for it).  On failure E is unspecified.  Synchronous. */
gdca_status gdca_energies_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q,
                              const int8_t *X_dev, int32_t K, double *E_dev);
/* Fused: fits the model on Z exactly as gdca_run does (theta, reweighting, tallies, pseudocount, covariance, the SPD inverse with its
 * conditioning screen, refinement, Cholesky fallback and second attempt -- the same code, so the model is bit for bit the one gdca_run
 * scores from), then computes the energies of X under it; mJ never leaves HBM.  X == NULL scores Z itself (K is then ignored and M
 * energies are written).  p->score and p->apc are ignored.  Status codes as gdca_run (GDCA_ENOTPD with st->info, ...).  Stats: everything
 * up to and including the inverse as a gdca_run of the same parameters reports it; ms_score is the energy stage, ms_fn 0, ms_total runs
 * to the end of the energy stage. */
gdca_status gdca_run_energies_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                  const int8_t *X_dev, int32_t K, double *E_dev, gdca_stats *st);

/* ---- log-likelihoods: log det C from the pivots of the inverse, normalised scores ---------------------------------------------------
 * The energies stop one constant short of a likelihood.  With it, the density of the continuous Gaussian N(Pi, C) at the one-hot point x:
 *     log p(x) = -E(x) - 1/2 (n log 2 pi + log det C),        n = N (q - 1)
 * and that is what makes models comparable: which of several families a sequence belongs to, which pseudocount gives the higher held-out
 * likelihood, how strongly the halves of a paired alignment co-vary (-1/2 (log det C - log det C_AA - log det C_BB)).
 * log det C costs nothing extra: the block sweep eliminates symmetrically without pivoting, so the scalar pivot d_i of its every step is
 * the square of the Cholesky diagonal, log det C = sum_i log d_i -- the quantity dpotrf would give.  Every SPD inverse of this library
 * leaves its n pivots in a vector of the context's workspace (a side output: the inverse itself is bit for bit what it was), and one
 * small kernel behind the inverse sums their logarithms in f64 in a fixed order (a fixed stride per thread, then a fixed tree; no
 * floating-point atomics; the identity padding is not summed).
 * Determinism: log det is the same bits from run to run for an inverse that has a launch of its own, and for the members of a merged
 * launch under option MERGE_GROUP=1 (their arithmetic is then that of a launch of their own); between different groupings of the sweep
 * (options GROUP, MERGE_GROUP, RAGGED) it agrees to rounding.  It does not depend on K or on X.
 * The conditioning branches: a second attempt of the sweep (st->sweep_retries) writes the pivots again and the value is that attempt's --
 * the undisturbed run's bits; after a Newton-Schulz step (st->refined = 1) the value stays that of the sweep's pivots: the step improves
 * the inverse, the pivots are backward stable as they are; after the Cholesky fallback (st->refined = 2, or option CHOLESKY=2) the value
 * is that of the fallback's diagonal, sum_i log L_ii^2, and `source` says so. */
#define GDCA_LOG_2PI 1.8378770664093453  /* log(2 pi), the nearest double */
/* log det of the matrix of the last SPD inverse this context completed: gdca_spd_inverse(_dev), a member of gdca_spd_inverse_batch_dev
 * (ask that member's context), or any fused run once it has been collected (gdca_run*, _energies, _pair_energies, _partner_match,
 * _mutation_scan, _loglik, the members of a phase batch).  k: after gdca_run_multi* the member index -- the value of the pseudocount group
 * of p[k] --, after a fused log-odds run (gdca_run_pair_logodds, gdca_run_partner_logodds) 0 = the joint C, 1 = C_AA, 2 = C_BB --,
 * 0 after everything else.  source (may be NULL): 0 = the sweep's pivots, 1 = the Cholesky fallback's diagonal.  Entry points
 * that take no inverse leave the record alone.  GDCA_EINVAL: no inverse yet (or the last one did not complete: GDCA_EHIP), k out of
 * range, a run outstanding on the context, a null pointer.  Where that inverse ended GDCA_ENOTPD the value is NaN, with GDCA_OK.  No device
 * work: the value came back with the inverse's other scalars. */
gdca_status gdca_last_logdet(gdca_ctx *ctx, int32_t k, double *logdet, int32_t *source);
/* gdca_spd_inverse(_dev) and the value in one call (logdet: a host pointer; NaN on failure).  The inverse is bit for bit
 * gdca_spd_inverse(_dev)'s, the status too. */
gdca_status gdca_spd_inverse_logdet_dev(gdca_ctx *ctx, double *A_dev, int32_t n, int32_t *info, double *logdet);
gdca_status gdca_spd_inverse_logdet(gdca_ctx *ctx, double *A, int32_t n, int32_t *info, double *logdet);
/* Fused: gdca_run_energies(_dev) unchanged (X == NULL scores Z itself, M values), then L[k] = -(E[k] + c) with
 *     c = 0.5 * (n * GDCA_LOG_2PI + logdet)
 * formed once on the host in plain f64 -- one multiplication, one addition, one multiplication, no contraction -- from the log det of the
 * inverse finally used (after a second attempt, refinement or fallback at collect time: see above), so L is bit for bit -(E + c) with E
 * from gdca_run_energies and logdet from gdca_last_logdet.  logdet (host pointer, may be NULL) receives that value.  Status codes and
 * stats as gdca_run_energies; ms_score includes the log det kernel and this epilogue.  On failure L is unspecified. */
gdca_status gdca_run_loglik_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                const int8_t *X_dev, int32_t K, double *L_dev, double *logdet, gdca_stats *st);
gdca_status gdca_run_loglik(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                            const int8_t *X_host, int32_t K, double *L_host, double *logdet, gdca_stats *st);

/* ---- pair energies: every pairing across a split alignment -----------------------------------------------------------------
 * Partner matching (the paper's second use of the model) takes an alignment of concatenated pairs A (+) B and needs, per species, the
 * energy of EVERY candidate pairing of K_A sequences of A with K_B of B.  Sites 0 .. split - 1 (0-based) are protein A, the rest
 * protein B, 1 <= split <= N - 1.  XA is split x K_A, XB is (N - split) x K_B, both int8 column-major with symbols 1..q like Z; E has
 * K_A K_B entries, column-major: E[a + K_A * b] (64-bit index).
 *     what = GDCA_PAIR_ENERGY:    E[a, b] = the energy gdca_energies gives the concatenation a (+) b,
 *     what = GDCA_PAIR_COUPLING:  R[a, b] = sum_{i in A, j in B, neither a gap} mJ[r(j), r(i)],  r(i) = i s + a_i - 1  (Pi may be NULL),
 * joined by the exact identity (g = mJ Pi, c0 = Pi' g; a gap leaves its site's block of the one-hot vector zero)
 *     E(a (+) b) = E(a (+) gaps) + E(gaps (+) b) - c0 / 2 + R(a, b).
 * The two marginal terms are K_A + K_B energies of the stage above; R reads ONE rectangular block of mJ -- rows n_A .. n - 1, columns
 * 0 .. n_A - 1, n_A = split (q - 1), inside the lower triangle -- and nothing else of it, at about N - split gathers a pairing where
 * the K_A K_B concatenations would cost N^2 / 2 each (and K_A K_B N bytes).  mJ as for gdca_energies: symmetric, lower triangle read.
 * Every sum is taken in a fixed order in f64 (no floating-point atomics): the bits of E[a, b] depend only on the model, a, b, split
 * and `what` -- not on K_A, K_B, where a and b stand in their batches, option PAIR_CHUNK (at most that many sequences of A per launch; 0 = the rule) or
 * the kernel instance.  An all-gap a or b has R = 0.0 exactly.
 * GDCA_EINVAL: K_A or K_B < 1, split outside 1..N-1, q outside 2..31, a null pointer that is needed, an unknown `what` -- nothing is
 * run -- or a byte of XA / XB outside 1..q (detected on the device; nothing is read out of bounds for it).  On failure E is unspecified.
 * Synchronous. */
enum { GDCA_PAIR_COUPLING = 0, GDCA_PAIR_ENERGY = 1 };
gdca_status gdca_pair_energies_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, int32_t split,
                                   const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, int32_t what, double *E_dev);
/* Fused: fits the model on Z exactly as gdca_run_energies does (the same code, the same conditioning screen), then the pair stage on
 * it; mJ never leaves HBM.  XA == NULL takes the A halves of Z's own sequences (K_A is then M, KA ignored); XB == NULL likewise and
 * independently, so both NULL gives the M x M matrix whose diagonal holds the native pairs.  p->score and p->apc are ignored.  Stats
 * as gdca_run_energies: ms_score is the pair stage, ms_fn 0. */
gdca_status gdca_run_pair_energies_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                       int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, int32_t what,
                                       double *E_dev, gdca_stats *st);

/* ---- partner matching per species: blocked pair energies and the assignment ---------------------------------------------------
 * A matching problem has many species with a handful of paralogs each: wanted are the pairings WITHIN a species, sum_s kA_s kB_s
 * entries, not K_A K_B.  The sequences of XA and of XB are SORTED BY SPECIES: species s = 0 .. S - 1 owns sequences offA[s] ..
 * offA[s + 1] - 1 of XA and offB[s] .. offB[s + 1] - 1 of XB.  offA and offB are HOST arrays of S + 1 int32 in every form (declared
 * const void * in the entry points), non-decreasing, offA[0] = offB[0] = 0, offA[S] = K_A, offB[S] = K_B; a species may be empty on
 * either side; S >= 1.  A violation is GDCA_EINVAL with nothing run.
 * The blocked matrix is packed: block s starts at eoff[s] = sum_{t < s} kA_t kB_t (64-bit) and is column-major kA_s x kB_s:
 *     E[eoff[s] + (a - offA[s]) + kA_s (b - offB[s])].
 * gdca_pair_blocks_length returns eoff[S], the doubles the packed matrix holds, or -1 for invalid offsets.
 *
 * gdca_pair_energies_blocked(_dev): `what` and every argument rule as gdca_pair_energies_dev (a bad symbol is detected on the
 * device).  EVERY ENTRY IS BIT FOR BIT the entry E[a + K_A b] gdca_pair_energies_dev writes for the same model, a, b, split and
 * `what`: the folded rows T[a][row] are summed over the A sites ascending by one thread, then gathered over the B sites ascending by
 * one thread, segments in ascending order, no floating-point atomics -- the fold, the pack, the pad and the marginal energies are the
 * full form's own; only the gather differs, spreading its lanes over the pairings of one species.  No limit on a species' size.
 *
 * gdca_assign_blocks(_dev): the minimum-cost one-to-one assignment inside every block of ANY blocked f64 cost matrix (energies or
 * couplings): per species min(kA_s, kB_s) pairs, shortest augmenting paths (Jonker-Volgenant) in f64, one workgroup a species.
 *     match[a] (int32, K_A entries)  the global index b of a's partner; -1 if a is unmatched (kA_s > kB_s, or kB_s = 0);
 *     gap[a]   (f64, K_A entries; may be NULL)  min_{b' != match(a)} E[a, b'] - E[a, match(a)], b' inside the species: ONE f64
 *              subtraction of two entries of E; +inf where kB_s = 1; +0.0 for an unmatched a; negative where the assignment
 *              overrode the row's own minimum.
 * Among optima of equal cost which one comes back is unspecified, but fixed for given input bits: run to run, and whatever other
 * species share the call.  Costs are meant to be finite: a species whose search runs out of finite entries (NaNs, infinities) comes
 * back unmatched as a whole (-1, +0.0).  GDCA_ASSIGN_MAX is the largest
 * kA_s or kB_s the assignment accepts: a larger species is GDCA_EINVAL with nothing run.  Synchronous. */
#define GDCA_ASSIGN_MAX 512
int64_t gdca_pair_blocks_length(const int32_t *offA, const int32_t *offB, int32_t S);
gdca_status gdca_pair_energies_blocked_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, int32_t split,
                                           const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, const void *offA,
                                           const void *offB, int32_t S, int32_t what, double *E_dev);
gdca_status gdca_assign_blocks_dev(gdca_ctx *ctx, const double *E_dev, const void *offA, const void *offB, int32_t S, int32_t *match_dev,
                                   double *gap_dev);
/* Fused: fits the model on Z exactly as gdca_run_pair_energies_dev does (the same code, the same conditioning screen), then the
 * blocked pair stage and the assignment on it.  XA == NULL or XB == NULL takes that half of Z's own sequences (the count is then M
 * and the offsets index Z).  E_dev == NULL keeps the blocked matrix in a grow-only buffer of the context.  Stats as
 * gdca_run_pair_energies: ms_score is the blocked pair stage plus the assignment. */
gdca_status gdca_run_partner_match_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                       int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB,
                                       const void *offA, const void *offB, int32_t S, int32_t what, double *E_dev, int32_t *match_dev,
                                       double *gap_dev, gdca_stats *st);

/* ---- pair log-odds: the joint model against the two marginal models, and matching on them ------------------------------------------
 * The partner score of the method (the paper's "protein-interaction partners") is the log-odds of a pairing under the joint model
 * against the two proteins modelled on their own:
 *     L(a, b) = log p_AB(a (+) b) - log p_A(a) - log p_B(b),      p_AB = N(Pi, C),  p_A = N(Pi_A, C_AA),  p_B = N(Pi_B, C_BB).
 * The joint energy ranks a pairing largely by how typical a and b each are; the log-odds removes exactly that part.
 * s = q - 1, n_A = split s, n_B = (N - split) s, n = n_A + n_B.  C is the covariance the fused run builds, Pi add_pseudocount's first
 * result, Pi_A = Pi[0 .. n_A), Pi_B = Pi[n_A .. n).  C_AA and C_BB are the diagonal blocks of THAT VERY C -- entry for entry its bits:
 * they share the joint alignment's weights, theta, Meff and pseudocount; they are not a refit on half the columns (which would
 * reweight differently).  The marginals' precisions are mJ_A = inv(C_AA), mJ_B = inv(C_BB): the TRUE marginals, not the diagonal
 * blocks of mJ = inv(C).
 *     EmA[a] = 1/2 (x_a - Pi_A)' mJ_A (x_a - Pi_A)     gdca_energies' rule with N = split and Pi_A; EmB[b] likewise with Pi_B
 *     E[a, b]                                          the joint energy: bit for bit gdca_(run_)pair_energies' with GDCA_PAIR_ENERGY
 *     ld, ldA, ldB                                     the three log dets, each from the pivots of its own inverse (or from the
 *                                                      fallback's diagonal where that inverse took the fallback)
 *     I = -0.5 * ((ld - ldA) - ldB)                    formed once, on the host, in plain f64, no contraction: the Gaussian mutual
 *                                                      information of the halves = the expected log-odds of a native pair (n log 2 pi
 *                                                      cancels).  Mathematically I >= 0; rounding can leave it a few ulps of ld
 *                                                      below zero (pseudocount 1: C is block diagonal).  It is not clamped.
 *     L[a, b] = ((EmA[a] + EmB[b]) - E[a, b]) + I      exactly these three f64 operations in this order: L[a, b] is bit for bit that
 *                                                      expression of the four values.  HIGHER = more likely partners.
 * The bits of L[a, b] depend only on the model, a, b and split -- not on K_A, K_B, positions in the batch, option PAIR_CHUNK or the
 * full or blocked form.  The gather kernels of the pair stage carry the combination in their epilogue (a third compile-time variant):
 * E is never stored, K_A K_B doubles are written once.
 *
 * gdca_pair_logodds(_dev): the operator form on the caller's three precisions (n x n, n_A x n_A, n_B x n_B: symmetric, lower triangle
 * read), Pi (n) and I; writes L[a + KA b].  Argument rules and the bad-symbol rule as gdca_pair_energies_dev.
 * gdca_pair_logodds_blocked(_dev): the same inside the species of species-sorted sequences; offA / offB / S and the packed layout as
 * gdca_pair_energies_blocked; every entry bit for bit the full form's.
 * gdca_run_pair_logodds(_dev): fused.  The front end runs once; then three fits one after the other -- C_AA, C_BB, C last -- each
 * through the SPD inverse with its conditioning screen, refinement, Cholesky fallback and second attempt as a single run of its own
 * size takes them; the marginal fits score their half's sequences, the joint fit the pairings.  XA == NULL or XB == NULL takes that
 * half of Z's own sequences, as gdca_run_pair_energies.  EmA_dev (K_A) and EmB_dev (K_B) are optional outputs.  info: optional HOST
 * array of GDCA_LOGODDS_FIELDS f64 by the GDCA_LOGODDS_* indices: the three log dets (NaN for a fit that did not complete), I, the
 * marginal fits' `refined` (as gdca_stats.refined), and -- 0 unless gdca_ctx_set_timing is on -- the device time of the two marginal
 * fits.  st: the joint fit's stats, exactly what gdca_run_pair_energies reports (ms_pair_tally: the tallies into Pij_true; ms_total
 * includes the marginal fits).  Afterwards gdca_last_logdet(ctx, k): k = 0 joint, 1 C_AA, 2 C_BB.
 * gdca_run_partner_logodds(_dev): the fused form, then the blocked form and the assignment.  Arguments as gdca_run_partner_match without
 * `what`, plus info.  The assignment MAXIMISES the total L inside every species (the minimum-cost assignment on -L; negation is
 * exact); gap[a] = L[a, match(a)] - max_{b' != match(a)} L[a, b'], ONE f64 subtraction of two entries of L, with gdca_assign_blocks'
 * special values: +inf where kB_s = 1, +0.0 for an unmatched a, negative where the assignment overrode the row's own best.
 * L_dev == NULL keeps the blocked matrix in a buffer of the context.  GDCA_ASSIGN_MAX applies.
 * Status: argument failures are GDCA_EINVAL with nothing run; a bad symbol is found on the device; where a fit fails (GDCA_ENOTPD, ..)
 * the call returns the status of the first failing fit in the order the fits run (A, B, joint) and L is unspecified.  A principal block
 * of a positive-definite matrix is positive definite, so a marginal fit can only fail where the joint one would.
 * The `what` values of the pair, partner and IPA entry points stay {0, 1}: the log-odds has entry points of its own. */
enum {
    GDCA_LOGODDS_LOGDET = 0, GDCA_LOGODDS_LOGDET_A, GDCA_LOGODDS_LOGDET_B, GDCA_LOGODDS_INFORMATION, GDCA_LOGODDS_REFINED_A,
    GDCA_LOGODDS_REFINED_B, GDCA_LOGODDS_MS_MARGINALS, GDCA_LOGODDS_RESERVED
};
#define GDCA_LOGODDS_FIELDS 8
gdca_status gdca_pair_logodds_dev(gdca_ctx *ctx, const double *mJ_dev, const double *mJA_dev, const double *mJB_dev, const double *Pi_dev,
                                  int32_t N, int32_t q, int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB,
                                  double I, double *L_dev);
gdca_status gdca_pair_logodds_blocked_dev(gdca_ctx *ctx, const double *mJ_dev, const double *mJA_dev, const double *mJB_dev,
                                          const double *Pi_dev, int32_t N, int32_t q, int32_t split, const int8_t *XA_dev, int32_t KA,
                                          const int8_t *XB_dev, int32_t KB, const void *offA, const void *offB, int32_t S, double I,
                                          double *L_dev);
gdca_status gdca_run_pair_logodds_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                      int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, double *L_dev,
                                      double *EmA_dev, double *EmB_dev, double *info, gdca_stats *st);
gdca_status gdca_run_partner_logodds_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                         int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB,
                                         const void *offA, const void *offB, int32_t S, double *L_dev, int32_t *match_dev,
                                         double *gap_dev, double *info, gdca_stats *st);

/* ---- iterative partner matching: grow the paired alignment on the device ----------------------------------------------------------
 * Who wants to pair paralogs usually has no trusted alignment of pairs to fit on: two pools with species labels, and a few certain
 * pairs.  The published procedure (progressive paralog matching, the iterative pairing algorithm) fits on the pairs trusted so far,
 * matches every species, keeps the most confident matches as the next training set -- a few more each round -- and repeats.
 * gdca_run_partner_ipa(_dev) is that loop, with the pools, the species table, the model and the growing alignment resident in HBM from
 * the first round to the last; the two entry points below are what it runs between two rounds.
 *
 * gdca_select_confident(_dev): match / gap as gdca_assign_blocks(_dev) returns them for KA sequences a.  The CANDIDATES are the a with
 * match[a] >= 0.  They are ordered by gap[a] descending under the total order of gdca_ranking (its 64-bit key: NaN first, then +inf,
 * 0.0 before -0.0), equal keys in ascending a; the first min(n_take, #candidates) are SELECTED (n_take <= 0: none).  sel (int32, KA
 * entries) receives the selected a in ASCENDING a and -1 from there on; *n_sel (host; may be NULL) their number.  Radix passes of the
 * ranking, a flag per a by rank, an exclusive scan, a compaction: no order-dependent atomics, the result is a function of the input
 * bits.  GDCA_EINVAL: KA < 1, a null pointer.  Synchronous.
 *
 * gdca_concat_pairs(_dev): writes columns col0 .. col0 + n_sel - 1 of Z (N x M int8, column-major, M >= col0 + n_sel: the caller's):
 * column col0 + t is XA[:, selA[t]] (split symbols) over XB[:, selB[t]] (N - split symbols).  One pass, a byte a thread.  An index
 * outside its pool is GDCA_EINVAL, detected on the device (nothing is read out of bounds for it; columns of valid indices may have
 * been written, nothing outside the requested columns is).  GDCA_EINVAL with nothing run: split outside 1..N - 1, KA or KB < 1,
 * n_sel or col0 < 0, a null pointer.  n_sel = 0 writes nothing.  Synchronous.
 *
 * gdca_run_partner_ipa(_dev): the pools XA (split x K_A) and XB ((N - split) x K_B) sorted by species, offA / offB / S exactly as for
 * gdca_run_partner_match; Zfix (N x Mfix; NULL with Mfix = 0): pairs that are part of EVERY round's training alignment; seedA / seedB
 * (n_seed HOST int32 each; may be empty): the first training set T_0 as index pairs into the pools.  Round r = 1, 2, ...:
 *     Z_r = [Zfix | the pairs (a, b) of T_{r-1} in ascending a]  (a grow-only buffer of the context; Zfix is copied once);
 *     fit on Z_r and match: gdca_run_partner_match's own code, so that ROUND r's match AND gap ARE BIT FOR BIT what
 *         gdca_run_partner_match returns for Z_r, the same pools and the same parameters (collect-time branches included);
 *     T_r = the selection of gdca_select_confident with n_take = r n_inc, each selected a paired with match[a].
 * The pairs are chosen afresh every round, not accumulated: a pool seed is replaced from round 1 on (a pair that is to stay belongs
 * into Zfix).  The loop ends after round max_rounds, after the first round r >= 2 whose training set already held every candidate of
 * the round before (n_sel of round r - 1 equalled its candidates), or -- Mfix = 0 only -- after a round that selects nothing.  The
 * offset checks, the species table, the gather's work list and the packed symbols of the pools with their symbol check are done once
 * per call; between two rounds only scalars cross PCIe (the fit's status block, the round's counts).
 *     match, gap (K_A entries; gap may be NULL)              the last completed round's
 *     match_trace, gap_trace (max_rounds x K_A; may be NULL)  round r's at row r - 1
 *     rounds_out (HOST f64, max_rounds x GDCA_IPA_FIELDS; may be NULL)  per round, by the GDCA_IPA_* indices: the columns of Z_r, the
 *         candidates, n_sel, the a whose match differs from the round before (round 1: the candidates), the fit's Meff, theta and
 *         log det C, the total cost sum over the candidates of E[a, match[a]] (f64, on the device: thread t takes a = t, t + 1024, ..
 *         ascending, then a fixed binary tree), and -- 0 unless gdca_ctx_set_timing is on -- ms_fit (front end and inverse), ms_match
 *         (blocked pair stage and assignment) and ms_select (the round's figures, its copies and the selection; the concatenation
 *         goes with the next round's front end)
 *     *rounds_run (HOST; may be NULL)  completed rounds;     st: the last fit's stats
 * GDCA_EINVAL with nothing run and no output touched: the checks of gdca_run_partner_match; Mfix + n_seed < 1; a seed index outside
 * its pool; a seed pair across two species; an a or a b twice in the seed; n_inc < 1 or max_rounds < 1; Mfix + K_A beyond INT32_MAX.
 * A bad symbol in a pool is GDCA_EINVAL before the first round.  If a round's fit fails (GDCA_ENOTPD, ..) that status is returned,
 * *rounds_run counts the completed rounds and match / gap are the last completed round's. */
enum {
    GDCA_IPA_M_TRAIN = 0, GDCA_IPA_CANDIDATES, GDCA_IPA_N_SEL, GDCA_IPA_N_CHANGED, GDCA_IPA_MEFF, GDCA_IPA_THETA, GDCA_IPA_LOGDET,
    GDCA_IPA_COST, GDCA_IPA_MS_FIT, GDCA_IPA_MS_MATCH, GDCA_IPA_MS_SELECT, GDCA_IPA_RESERVED
};
#define GDCA_IPA_FIELDS 12
gdca_status gdca_select_confident_dev(gdca_ctx *ctx, const int32_t *match_dev, const double *gap_dev, int32_t KA, int32_t n_take,
                                      int32_t *sel_dev, int32_t *n_sel);
gdca_status gdca_concat_pairs_dev(gdca_ctx *ctx, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, int32_t N, int32_t split,
                                  const int32_t *selA_dev, const int32_t *selB_dev, int32_t n_sel, int8_t *Z_dev, int32_t col0);
gdca_status gdca_run_partner_ipa_dev(gdca_ctx *ctx, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, const void *offA,
                                     const void *offB, int32_t S, int32_t N, int32_t q, int32_t split, int32_t what, const gdca_params *p,
                                     const int8_t *Zfix_dev, int32_t Mfix, const int32_t *seedA, const int32_t *seedB, int32_t n_seed,
                                     int32_t n_inc, int32_t max_rounds, int32_t *match_dev, double *gap_dev, int32_t *match_trace_dev,
                                     double *gap_trace_dev, double *rounds_out, int32_t *rounds_run, gdca_stats *st);

/* ---- mutation scan: the energy change of every single substitution ---------------------------------------------------------
 * The mutational landscape of a sequence under the model (what is compared with deep mutational scans).  Conventions as for the
 * energies above: s = q - 1, n = N s, r(i, c) = i s + c - 1 for symbol c in 1..s at 0-based site i, the gap q has no row, Pi is
 * add_pseudocount's first result, g = mJ Pi.  For a sequence x (N symbols), a site i and a symbol c the SITE POTENTIAL is
 *     V(x; i, c) = sum over the sites j != i with x_j no gap of mJ[r(i,c), r(j,x_j)]  +  1/2 mJ[r(i,c), r(i,c)]  -  g[r(i,c)],   c in 1..s,
 *     V(x; i, q) = 0   (exactly +0.0),
 * and E(x with site i set to c) = V(x; i, c) + a term that does not depend on c, so the energy change of the substitution x_i -> b is
 *     dE(x; i, b) = V(x; i, b) - V(x; i, x_i)
 * -- the gdca_energies energy of the mutant minus that of x up to rounding -- at N gathers an entry where the explicit mutant costs
 * N^2 / 2; no mutant is written down.
 *     what = GDCA_MUT_POTENTIAL:  D = V,
 *     what = GDCA_MUT_DELTA:      D = dE, ONE f64 subtraction of the two potentials the other mode returns: D[k, i, b] is bit-equal to
 *                                 V[k, i, b] - V[k, i, x_i], and the entry b = x_i is exactly +0.0.
 * X is N x K int8 column-major like Z, K >= 1.  D has q N K doubles, column-major q x N x K: D[(b - 1) + q (i + N k)] (64-bit index;
 * a (K, N, q) array in row-major terms); column q is the gap target ("delete this residue").  mJ as for gdca_energies: symmetric,
 * only its lower triangle is read.  Every sum is taken in a fixed order in f64 (no floating-point atomics): the bits of D[k, i, :]
 * depend only on the model, x_k and `what` -- not on K, on where x_k stands in the batch or on the kernel instance.
 * GDCA_EINVAL: K < 1 or K > INT32_MAX - 256, q outside 2..31, an unknown `what`, a null pointer -- nothing is run -- or a byte of X outside 1..q (detected on
 * the device; nothing is read out of bounds for it).  On failure D is unspecified.  Synchronous. */
enum { GDCA_MUT_DELTA = 0, GDCA_MUT_POTENTIAL = 1 };
gdca_status gdca_mutation_scan_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                   int32_t K, int32_t what, double *D_dev);
/* Fused: fits the model on Z exactly as gdca_run_energies does (the same code, the same conditioning screen), then the scan on it; mJ
 * never leaves HBM.  X == NULL scans Z's own M sequences (K is then ignored and q N M doubles are written).  p->score and p->apc are
 * ignored.  Stats as gdca_run_energies: ms_score is the scan stage, ms_fn 0. */
gdca_status gdca_run_mutation_scan_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                       const int8_t *X_dev, int32_t K, int32_t what, double *D_dev, gdca_stats *st);

/* ---- double-mutant scan: epistasis and the best double substitution of every site pair ------------------------------------
 * The double-mutant landscape of a sequence under the model (what is compared with double-mutant libraries; which second
 * substitution rescues a first one).  Conventions as in the mutation-scan section above: s, n, r(i, c), the gap q has no row, only the
 * lower triangle of mJ is read.  No double mutant is written down: for a wild type x, sites i != j and targets b (at i), c (at j)
 *     E(x with i -> b, j -> c) - E(x) = dE(x; i, b) + dE(x; j, c) + eps(x; i, b; j, c),
 *     eps(x; i, b; j, c) = K(i,b; j,c) - K(i,x_i; j,c) - K(i,b; j,x_j) + K(i,x_i; j,x_j),      K(i,b; j,c) = mJ[r(i,b), r(j,c)],
 * K = 0 where b or c is the gap.  eps is the EPISTASIS of the two substitutions in the background x.
 * DEFINITIONS (everything below refers to these).  Orientation: i < j, a = x_i, a' = x_j.  B[b,c] = mJ[r(i,b), r(j,c)], exactly +0.0
 * where b == q or c == q.  dE denotes the bits gdca_mutation_scan(.., GDCA_MUT_DELTA) returns for x.  The fixed f64 expressions:
 *     eps[b,c] = (B[b,c] - B[a,c]) - (B[b,a'] - B[a,a'])
 *     ddE[b,c] = (dE[i,b] + dE[j,c]) + eps[b,c]
 * With this grouping eps is exactly 0 when b == a or c == a'.  (The fused forms read -mJ; every difference negates exactly, so they
 * return the same bits as the operator forms on the same model.)
 * MAPS, per sequence k: N x N x K entries each, column-major, index i + N (j + N k) (64-bit), both triangles filled:
 *     Emin (f64)    min of ddE[b,c] over the admissible targets b != x_i, c != x_j, b and c in 1..q: the gap target ("delete") is
 *                   included, a gap site may receive any residue -- the most stabilising true double substitution of the pair;
 *     code (int32)  its minimiser as (b - 1) + q (c - 1) in the orientation i < j; ties go to the smallest code (ONE thread walks the
 *                   codes in ascending order with a strict <); entry [j,i,k] holds the same pair transposed, (c - 1) + q (b - 1);
 *     epi (f64)     the epistasis strength of the pair in this background, sqrt(sum over all q^2 targets of eps[b,c]^2), summed by one
 *                   thread in ascending code order (a rounded product and a rounded sum a code).
 * Emin[j,i,k] and epi[j,i,k] are the bits of [i,j,k].  Diagonal entries: Emin = +0.0, code = -1, epi = +0.0.  Any of the three
 * pointers may be NULL: that map is skipped; all three NULL is GDCA_EINVAL.
 * LISTED DOUBLE MUTANTS (the form one compares with an experimental library): muts holds L records of five int32 (k, i, b, j, c),
 * column-major 5 x L, sites 0-based, symbols in 1..q; out[l] = ddE[b,c] of record l once it is put into the orientation i < j -- it
 * does not matter which substitution is named first.  b == x_i or c == x_j is allowed: the result is then bit for bit the dE of the
 * other site (+0.0 if both match).
 * X is N x K int8 column-major, K >= 1, and must be given (there is no "scan Z itself" form: N^2 M outputs).  The bits of every
 * output entry depend only on the model and x_k -- not on K, on where x_k stands in the batch, on the kernel instance or on fused /
 * operator.  The stage keeps dE of all K sequences in a context workspace of q N K doubles.
 * GDCA_EINVAL: N < 2, q outside 2..31, K < 1 or K > INT32_MAX - 256, ceil(K / 64) T (T + 1) / 2 > 2^24 with T = ceil(N / 4), L < 1,
 * a null pointer (X included) -- nothing is run -- or, detected on the device with nothing indexed by it: a byte of X outside 1..q,
 * a record with i == j or with k, i, j, b or c out of range.  On failure the outputs are unspecified.  Synchronous. */
gdca_status gdca_double_mutant_scan_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                        int32_t K, double *Emin_dev, int32_t *code_dev, double *epi_dev);
gdca_status gdca_double_mutants_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                    int32_t K, const void *muts_dev, int32_t L, double *out_dev);
/* Fused, exactly as gdca_run_mutation_scan (the fit, the conditioning screen, a refinement or fallback at collect time runs the stage
 * again) but X must be given.  Stats: ms_score is the stage (the single-substitution scan and the double-mutant kernel), ms_fn 0. */
gdca_status gdca_run_double_mutant_scan_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                            const int8_t *X_dev, int32_t K, double *Emin_dev, int32_t *code_dev, double *epi_dev,
                                            gdca_stats *st);
gdca_status gdca_run_double_mutants_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                        const int8_t *X_dev, int32_t K, const void *muts_dev, int32_t L, double *out_dev, gdca_stats *st);

/* ---- greedy walk: every sequence descends to a local energy minimum, one substitution a step -------------------------------
 * From a wild type take the most stabilising single substitution, update the landscape, repeat -- for max_steps steps or until no
 * substitution lowers the energy: the greedy k-fold mutant, the local minimum a sequence drains to, and how far above it the
 * sequence sits.  Conventions as in the mutation-scan section above: s, n, r(i, c), the gap q has no row, only the lower triangle of
 * mJ is read; K(j,c; i,b) = mJ[r(j,c), r(i,b)], exactly +0.0 where b == q.  (The fused forms read -mJ; every expression below negates
 * exactly, so they return the same bits as the operator forms on the same model.)
 * STATE per sequence: the current symbols x (N) and a table V[i][c], c in 1..q; V[i][q] is +0.0 and never written.  Start:
 * x = X[:, k] and V = the bits gdca_mutation_scan(.., GDCA_MUT_POTENTIAL) returns for that sequence.
 * ADMISSIBLE MOVES in state x: site i if mask == NULL or mask[i] != 0 -- and, where x_i == q, only with GDCA_WALK_FILL_GAPS --, to a
 * target b in 1..q, b != x_i; b == q only with GDCA_WALK_GAP_TARGET.  flags = 0: residues change into residues, gaps stay gaps.
 * STEP: dE(i, b) = V[i][b] - V[i][x_i], ONE f64 subtraction of two table entries.  The step takes the admissible (i, b) that minimises
 * dE, ties to the smallest code i q + (b - 1) (the total order on (dE, code): any reduction tree gives the same result; a NaN dE is
 * never chosen).  The walk stops if there is no admissible move, if the best move does not satisfy dE < -min_gain, or after
 * max_steps steps.  Otherwise it records (i, b, dE), sets x_i = b (a the old symbol), and for every site j != i and every c in 1..s
 *     V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a))                         (one subtraction, then one addition);
 * site i's own row is not touched: V(x; i, .) does not depend on x_i.
 * In exact arithmetic the energy falls strictly, so a walk ends.  The table is updated in f64 and drifts from the potentials of the
 * current sequence by about one unit roundoff of its entries a step; with min_gain = 0 two moves worth about 1e-16 could in
 * principle alternate.  max_steps bounds that, and a min_gain above the drift (1e-9 is far above it for |V| ~ 1e2) rules it out.
 * OUTPUTS (K sequences, X N x K int8 column-major):
 *     Xout     N x K int8: the final sequences; must not overlap X or Z;
 *     steps    K int32: the steps taken;
 *     dE_sum   K f64: the sum of the recorded dE in step order (one thread); may be NULL;
 *     path     2 x max_steps x K int32, column-major: record t of sequence k is (i, b), i 0-based, b in 1..q; the rows from steps[k]
 *              on hold -1; may be NULL;
 *     dE_path  max_steps x K f64; the rows from steps[k] on hold +0.0; may be NULL;
 *     V        q x N x K f64 in gdca_mutation_scan's layout: the FINAL table as the walk left it; may be NULL.
 * mask: N int8 shared by all sequences, NULL = every site may change.  The bits of everything a walk returns depend on the initial
 * table's bits, the model, x_k, mask, flags, min_gain and max_steps -- not on K, on where x_k stands in the batch, on the kernel
 * instance or on where the table lives (context option WALK_TABLE).  No floating-point atomics.  Without V the stage keeps the tables
 * in the double-mutant scan's context workspace of q N K doubles.
 * GDCA_EINVAL: K < 1 or K > INT32_MAX - 256, q outside 2..31, max_steps outside 1..GDCA_WALK_MAX_STEPS, min_gain < 0 or NaN, a
 * flags bit other than the two, a null X (operator form), Xout or steps, WALK_TABLE = lds with a table that does not fit -- nothing
 * is run -- or a byte of X outside 1..q (detected on the device before anything is indexed with it).  On failure the outputs are
 * unspecified.  Synchronous. */
enum { GDCA_WALK_GAP_TARGET = 1, GDCA_WALK_FILL_GAPS = 2 };
#define GDCA_WALK_MAX_STEPS 65535
gdca_status gdca_greedy_walk_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                 int32_t K, const int8_t *mask_dev, int32_t flags, double min_gain, int32_t max_steps, int8_t *Xout_dev,
                                 int32_t *steps_dev, double *dE_sum_dev, int32_t *path_dev, double *dE_path_dev, double *V_dev);
/* Fused, exactly as gdca_run_mutation_scan (the fit, the conditioning screen; a refinement or fallback at collect time runs the stage
 * again).  X == NULL walks Z's own M sequences (K is then ignored).  p->score and p->apc are ignored.  Stats: ms_score is the stage
 * (the scan and the walk), ms_fn 0. */
gdca_status gdca_run_greedy_walk_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                     const int8_t *X_dev, int32_t K, const int8_t *mask_dev, int32_t flags, double min_gain,
                                     int32_t max_steps, int8_t *Xout_dev, int32_t *steps_dev, double *dE_sum_dev, int32_t *path_dev,
                                     double *dE_path_dev, double *V_dev, gdca_stats *st);

/* ---- Metropolis chains: sequences drawn from the model at an inverse temperature beta ------------------------------------------
 * K chains, each a Markov chain of single substitutions whose stationary distribution is exp(-beta E(x)) / Z over its state space:
 * artificial homologues, a thermal ensemble around a wild type, an annealing step (a caller chains calls with the final table V).
 * Conventions as in the greedy-walk section: s = q - 1, r(i, c), the gap q has no row and V[i][q] = +0.0, only the lower triangle of
 * mJ is read, K(j,c; i,b) = mJ[r(j,c), r(i,b)] and +0.0 where b == q; the fused forms read -mJ and negate exactly.
 * STATE per chain: the current symbols x (N) and the table V, which starts as the bits gdca_mutation_scan(.., GDCA_MUT_POTENTIAL)
 * returns for the start sequence X[:, k].
 * STATE SPACE.  flags = 0: residues change into residues, gaps stay gaps.  GDCA_SAMPLE_GAPS: the gap is a symbol like any other.  No
 * other flag bit exists (the walk's two one-way flags would break detailed balance).  T = the number of target symbols: s without
 * the flag, q with it.  sites = the ascending list of the sites i with mask == NULL or mask[i] != 0 and -- without the flag --
 * x_i != q; it cannot change along a chain.  n_sites == 0: nothing is ever accepted and every sample is the start.
 * RANDOM NUMBERS: counter-based SplitMix64 with random access, all arithmetic mod 2^64, G = 0x9E3779B97F4A7C15:
 *     mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
 *     key(seed, stream) = mix64(mix64(seed + G) + (stream + 1) * G)
 *     draw(key, c)      = mix64(key + (c + 1) * G),  c = 0, 1, 2, ...
 * Chain k of a call uses stream = stream0 + k; proposal t (0-based, counted over the whole chain) uses r0 = draw(key, 2 t) and
 * r1 = draw(key, 2 t + 1).  Known answers: key(0, 0) = 0xa706dd2f4d197e6f with the draws 0x238275bc38fcbe91, 0xf89a2566b5822c54,
 * 0x47200e1d9780fa44; key(1, 0) = 0x5e41ab087439611e with 0xb18a02f46d8d86c3, 0xf8c5b62c83f707e8; key(1, 5) = 0xc63f062c5c30e3d4
 * with 0xfdba48dbc8c4fa9a; key(2^64 - 1, 2^63) = 0xf7f1454e6a8a1fa6 with 0xe447897adec0a36e.
 * A PROPOSAL: m = ((r0 >> 32) * n_sites) >> 32 and i = sites[m]; v = ((r0 & 0xffffffff) * (T - 1)) >> 32; a = the 0-based symbol of
 * x_i; the target is b = v + (v >= a), uniform over the T - 1 other symbols (the bias of either multiply-shift is below
 * 2^-32 max(n_sites, T)).  u = ((r1 >> 11) + 1) * 2^-53, in (0, 1]; thr = -log(u), the one transcendental of a step.
 * dE = V[i][b] - V[i][a], ONE f64 subtraction as in the walk.  ACCEPT iff beta * dE <= thr: one f64 multiplication, one comparison; a
 * NaN on the left never accepts; at beta = 0 every finite dE accepts.  On acceptance x_i = b, dE is added to the chain's running sum
 * (one thread, step order), and every other site's potentials are updated with the walk's two operations,
 *     V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a)),  j != i, c in 1..s;                 site i's own row is not touched.
 * LENGTH: n_steps = burn + n_samples * stride proposals, burn >= 0, stride >= 1, n_samples >= 1, n_steps <= INT32_MAX.  Sample j
 * is the state after proposal burn + (j + 1) * stride - 1.
 * OUTPUTS (K chains, X N x K int8 column-major):
 *     Xs        N x n_samples x K int8, column-major: sample j of chain k is the N bytes at ((k * n_samples) + j) * N -- itself an
 *               N x (n_samples K) alignment, as gdca_energies or gdca_frequencies take one; must not overlap X or Z;
 *     dE_s      n_samples x K f64: the running sum of the accepted dE at the moment of the sample, so E(sample) ~ E(start) + dE_s;
 *               may be NULL;
 *     accepted  K int32: the accepted proposals over all n_steps;
 *     thr       n_steps x K f64: the thresholds as the device computed them; may be NULL;
 *     moves     n_steps x K int32: the proposal's code i q + b (b 0-based, the walk's code) if accepted, -1 - code if rejected,
 *               INT32_MIN where n_sites == 0; may be NULL;
 *     V         q x N x K f64 in gdca_mutation_scan's layout: the final table; may be NULL.
 * ORDER: one thread updates an entry, one thread keeps the sum, the random numbers are functions of (seed, stream, t), no
 * floating-point atomics.  The bits of everything a chain returns depend on the initial table's bits, the model, x_k, mask, flags,
 * beta, seed, the chain's stream number, burn, stride, n_samples and the values of thr -- not on K or where the chain stands in the
 * batch (a batch stream0 .. stream0 + K - 1 is its chains run one at a time with stream0 + k), on where the table lives (context
 * option WALK_TABLE, shared with the walk), or on how the chain is cut into launches (context option SAMPLE_CHUNK).  Without V the
 * stage keeps the tables in the double-mutant scan's context workspace of q N K doubles.
 * GDCA_EINVAL, nothing run: K < 1 or K > INT32_MAX - 256, q outside 2..31, T < 2 (q = 2 without the flag), beta < 0, NaN or
 * infinite, burn < 0, stride < 1, n_samples < 1, n_steps > INT32_MAX, a flags bit other than GDCA_SAMPLE_GAPS, a null X (operator
 * form), Xs or accepted, WALK_TABLE = lds with a table that does not fit, N > GDCA_SAMPLE_MAX_SITES (the site list is kept in LDS).  A byte of X
 * outside 1..q is detected on the device before anything is indexed with it.  On failure the outputs are unspecified.  Synchronous. */
enum { GDCA_SAMPLE_GAPS = 1 };
#define GDCA_SAMPLE_MAX_SITES 54000
gdca_status gdca_sample_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev, int32_t K,
                            const int8_t *mask_dev, int32_t flags, double beta, uint64_t seed, uint64_t stream0, int32_t burn,
                            int32_t stride, int32_t n_samples, int8_t *Xs_dev, double *dE_s_dev, int32_t *accepted_dev, double *thr_dev,
                            int32_t *moves_dev, double *V_dev);
/* Fused, exactly as gdca_run_greedy_walk_dev (a refinement or fallback at collect time samples again on the inverse finally used).
 * X == NULL starts one chain from each of Z's own M sequences (K is then ignored).  Stats: ms_score is the stage (the scan and the
 * chains), ms_fn 0. */
gdca_status gdca_run_sample_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                const int8_t *X_dev, int32_t K, const int8_t *mask_dev, int32_t flags, double beta, uint64_t seed,
                                uint64_t stream0, int32_t burn, int32_t stride, int32_t n_samples, int8_t *Xs_dev, double *dE_s_dev,
                                int32_t *accepted_dev, double *thr_dev, int32_t *moves_dev, double *V_dev, gdca_stats *st);

/* ---- Replica-exchange chains: the Metropolis chains tempered over a ladder of inverse temperatures --------------------------------
 * Single-substitution chains at beta = 1 mix slowly on a fitted model.  Replica exchange (parallel tempering) runs R copies of every
 * chain at a ladder of inverse temperatures and lets neighbouring temperatures swap by a Metropolis rule: the hot copies cross
 * barriers, the swaps carry their states down, only the copy at the target temperature is sampled.  Conventions, state space,
 * flags, mask, proposal, `beta * dE <= thr`, table update and generator (mix64, key, draw) are the Metropolis-chain section's.
 * REPLICAS.  Chain k (0 .. K - 1) has R replicas, 1 <= R <= GDCA_TEMPER_MAX.  betas: a HOST array of R f64, each finite and >= 0, in
 * any order; betas[0] is the target temperature and the only one sampled; the slots p and p + 1 are swap partners.  A replica HOLDS a
 * slot; the states and tables never move, a swap exchanges the slots of two replicas.
 * START.  Xr is N x R x K int8: replica (k, r) is the N bytes at (k R + r) N.  slot0 is R x K int32 (slot0[r + R k] = the slot replica
 * r holds) or NULL: replica r holds slot r.  Every column of slot0 must be a permutation of 0 .. R - 1; that is checked on the device
 * before anything is indexed with it (GDCA_EINVAL).  A replica's table starts as the bits gdca_mutation_scan(.., GDCA_MUT_POTENTIAL)
 * returns for its start, E0[k, r] is the bits gdca_energies_dev returns for it, its site list is that of its own start.
 * STREAMS.  Replica (k, r) draws its proposals from stream0 + k R + r exactly as a plain chain on that stream would: the stream belongs
 * to the replica (the state), not to the temperature.  K R and the stream range obey gdca_sample_dev's limits for K.
 * PROPOSALS.  Proposal t of a replica is the Metropolis section's proposal t with beta = betas[the slot held]; the running sum S of
 * its accepted dE is one thread's, in step order.
 * SWAP ROUND e (e = 0, 1, ..) takes place after proposal t of every replica whenever (t + 1) % swap_every == 0, swap_every >= 1.  It
 * attempts the pairs p in 0 .. R - 2 with p % 2 == e % 2 (disjoint).  For pair p: a = the replica holding slot p, b = the one holding
 * p + 1; Ea = E0[a] + S[a], Eb = E0[b] + S[b] (one addition each); d = (betas[p] - betas[p + 1]) * (Eb - Ea): two subtractions, one
 * multiplication, no contraction; u = ((draw(skey_k, e R + p) >> 11) + 1) * 2^-53 with skey_k = mix64(~key(seed, stream0 + k R));
 * thr_s = -log(u).  ACCEPT iff d <= thr_s: a NaN never accepts, equal betas accept every finite d.  On acceptance a and b exchange
 * slots.  Known answers: skey of (seed, stream0, k, R) = (0, 0, 0, 3) is 0x1c44fab6a246bae2 with draw(skey, 0) = 0x3dc548297666b4b4
 * (round 0, pair 0) and draw(skey, 4) = 0xace4d333b149e3d1 (round 1, pair 1); of (1, 5, 2, 4) it is 0x56a6a56ca201d633 with
 * 0x9faf955cbe491e47 and draw(skey, 5) = 0xf81e54a1e15977ed.
 * SAMPLES.  burn % swap_every == 0 and stride % swap_every == 0, so that every sample point coincides with a round: sample j is the
 * state of slot 0's holder after the round at proposal burn + (j + 1) stride - 1.  n_steps = burn + n_samples stride,
 * n_rounds = n_steps / swap_every.
 * OUTPUTS (column-major):
 *     Xs         N x n_samples x K int8, gdca_sample_dev's layout;
 *     E_s        n_samples x K f64: E0 + S of the holder at the sample (one addition); may be NULL;
 *     accepted   R x K int32: accepted proposals, counted BY THE SLOT held when proposed;
 *     swaps      (R - 1) x K int32: accepted swaps per pair (the attempts are a function of e alone); not NULL even where R == 1;
 *     Xr_out     N x R x K int8: the final states; may alias nothing that is read;
 *     slot_out   R x K int32: the final slots (Xr_out and slot_out continue a run as Xr and slot0);
 *     thr, moves n_steps x R x K, by replica, gdca_sample_dev's meaning; each may be NULL;
 *     swap_thr   n_rounds x (R - 1) x K f64: thr_s, +0.0 for a pair not attempted in that round; may be NULL;
 *     slot_path  n_rounds x R x K int32: the slot of every replica after the round; may be NULL.
 * ORDER: no floating-point atomics, no reduction whose order depends on the launch.  The bits of everything returned for chain k
 * depend on the model, its starts, slot0, mask, flags, betas, seed, its stream numbers, burn, stride, n_samples, swap_every and the
 * values of thr and swap_thr -- not on K, on where the chain stands in the batch, on WALK_TABLE or on SAMPLE_CHUNK.
 * R = 1 is gdca_sample_dev on stream stream0 + k, bit for bit: Xs, accepted, thr, moves equal, E_s = E0 + dE_s (one addition),
 * whatever swap_every divides burn and stride.
 * GDCA_EINVAL, nothing run: everything gdca_sample_dev refuses with K R in the place of K; R outside 1 .. GDCA_TEMPER_MAX; a beta
 * negative, NaN or infinite; swap_every < 1 or one that does not divide burn and stride; a null Xr (operator form), Xs, accepted,
 * swaps, Xr_out, slot_out or betas.  A byte of Xr outside 1..q is detected on the device as in the chains.  The tables live in the
 * context's workspace of q N K R doubles.  Synchronous. */
#define GDCA_TEMPER_MAX 64
gdca_status gdca_sample_tempered_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *Xr_dev,
                                     const int32_t *slot0_dev, int32_t K, int32_t R, const double *betas, const int8_t *mask_dev,
                                     int32_t flags, uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride,
                                     int32_t n_samples, int8_t *Xs_dev, double *E_s_dev, int32_t *accepted_dev, int32_t *swaps_dev,
                                     int8_t *Xr_out_dev, int32_t *slot_out_dev, double *thr_dev, int32_t *moves_dev, double *swap_thr_dev,
                                     int32_t *slot_path_dev);
/* Fused, exactly as gdca_run_sample_dev: X is N x K, or NULL for Z's own M sequences (K is then ignored); every replica of a chain
 * starts at that chain's sequence and replica r holds slot r. */
gdca_status gdca_run_sample_tempered_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                         const int8_t *X_dev, int32_t K, int32_t R, const double *betas, const int8_t *mask_dev,
                                         int32_t flags, uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride,
                                         int32_t n_samples, int8_t *Xs_dev, double *E_s_dev, int32_t *accepted_dev, int32_t *swaps_dev,
                                         int8_t *Xr_out_dev, int32_t *slot_out_dev, double *thr_dev, int32_t *moves_dev,
                                         double *swap_thr_dev, int32_t *slot_path_dev, gdca_stats *st);

/* ---- Log partition function (annealed importance sampling) ---------------------------------------------------------------------------
 * The discrete models -- (W, zeros) of gdca_bm_learn* and gdca_plm_learn*, and (mJ, Pi) read as a Potts model by the chains -- have
 * energies without a normaliser.  Annealed importance sampling (Neal 2001) estimates log Z(beta) = log sum_{x in Omega} exp(-beta E(x)):
 * K chains start at uniform draws from Omega, run the Metropolis chain along a ladder of inverse temperatures from 0 to beta, and
 * carry the product of the ratios exp(-(betas[l] - betas[l-1]) E) met on the way; |Omega| mean_k(w_k) is an unbiased estimate of Z
 * for any ladder and any number of proposals a stage.  With it -E(x) - log Z is a log-likelihood, and S = log Z + <E> the
 * model's entropy.  Conventions, flags, mask, `sites`, T, proposal, `beta * dE <= thr`, table update and generator (mix64, key, draw)
 * are the Metropolis-chain section's.
 * STATE SPACE Omega.  A template x (N int8) fixes what does not move: sites = the template's site list (mask, and without
 * GDCA_SAMPLE_GAPS the template's gaps stay gaps), |Omega| = T^n_sites.  x == NULL is allowed only with mask == NULL and means that
 * every site is free.
 * LADDER.  betas: a HOST array of L + 1 f64, L >= 1; betas[0] must be exactly 0 (the base distribution is the uniform one); every
 * entry finite and >= 0; monotonicity is not required; betas[L] is the temperature whose Z is estimated.  The array is uploaded into a
 * grow-only context buffer (a ladder may be far longer than GDCA_TEMPER_MAX).
 * START of chain k (K chains, stream stream0 + k).  ikey = mix64(~key(seed, stream0 + k)) (the replica-exchange section's skey: no
 * swaps exist here).  The site at list position m gets the 0-based symbol ((draw(ikey, m) >> 32) * T) >> 32; every other site keeps the
 * template's symbol.  Known answers: (seed, stream) = (0, 0) has ikey = 0x1c44fab6a246bae2; m = 0 draws 0x3dc548297666b4b4: 0-based
 * symbol 0 at T = 3, 0 at T = 4, 4 at T = 20, 5 at T = 21; m = 4 draws 0xace4d333b149e3d1: 2, 2, 13, 14; m = 69 draws
 * 0x8537d76ccb32cd7e: 1, 2, 10, 10.
 * START TABLE AND ENERGY.  V0 = the bits gdca_mutation_scan(.., GDCA_MUT_POTENTIAL) returns for the start, E0 = the bits
 * gdca_energies_dev returns for it (the replica-exchange section's pairing).
 * STAGES l = 1 .. L, each of sweep >= 1 proposals; all arithmetic f64, one rounding an operation, no contraction.
 *     weight step   E = E0 + S, S the running sum of the accepted dE at that moment (+0.0 ahead of stage 1);
 *                   logw = logw + (betas[l-1] - betas[l]) * E: one subtraction, one multiplication, one addition; logw starts at +0.0;
 *     proposals     t = (l - 1) sweep .. l sweep - 1, exactly the Metropolis section's proposal t, at beta = betas[l].
 * n_steps = L * sweep <= INT32_MAX.  E_end = E0 + S after the last proposal.  One thread keeps logw, as one thread keeps S.
 * REDUCTION (out4), on the device in a fixed order, no floating-point atomics:  m = max_k logw[k];  e_k = exp(logw[k] - m);
 * S1 = sum e_k and S2 = sum e_k * e_k, each summed as gdca_bm_readout_dev sums (256 strided partials, partial t the terms
 * k = t, t + 256, .. ascending added to +0.0, folded by the halving tree t and t + 128, t and t + 64, ..);
 * log_omega = (double)n_sites * log((double)T);
 *     out[0] = log_omega + (m + log(S1 / (double)K))     the estimate of log Z(betas[L]) over Omega
 *     out[1] = S1 * S1 / S2                              the effective sample size, in [1, K]
 *     out[2] = m                                         out[3] = log_omega
 * Any non-finite logw[k] makes out[0] and out[1] NaN.  exp and log are the device library's: their bits are not pinned.
 * OUTPUTS (column-major).  Required: out4 (4 f64), logw (K f64).  Optional, each may be NULL: E_end (K f64); X0 (N x K int8, the
 * starts); Xout (N x K int8, the final states: with logw a weighted sample of the target); accepted (K int32); thr, moves (n_steps x K,
 * gdca_sample_dev's meaning).
 * ORDER: the bits depend on the model, the template, mask, flags, betas, sweep, seed, the chain's stream number and the values of thr
 * -- not on where the chain stands in the batch, on WALK_TABLE or on SAMPLE_CHUNK (a cut may fall inside a stage).  logw[k] and the
 * traces do not depend on K; out4 depends on K by definition and is the same bits from run to run.
 * GDCA_EINVAL, nothing run: whatever gdca_sample_dev refuses for K, q, flags, N and the table's placement, and T < 2; L < 1 or
 * sweep < 1; L * sweep > INT32_MAX; betas[0] != 0, or a beta negative, NaN or infinite; a null betas, out4 or logw; x == NULL together
 * with a mask.  A template byte outside 1..q is detected on the device as in the chains (such a site is never free).  The tables live
 * in the context's workspace of q N K doubles.  Synchronous.  New symbols only: gdca_stats and gdca_params are unchanged.  There is no
 * fused gdca_run_* form (as with gdca_bm_learn_dev the users are fitted Potts models). */
gdca_status gdca_log_partition_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *x_dev,
                                   const int8_t *mask_dev, int32_t flags, const double *betas, int32_t L, int32_t sweep, int32_t K,
                                   uint64_t seed, uint64_t stream0, double *out4_dev, double *logw_dev, double *E_end_dev, int8_t *X0_dev,
                                   int8_t *Xout_dev, int32_t *accepted_dev, double *thr_dev, int32_t *moves_dev);
/* ... with host pointers: upload, the _dev form, download */
gdca_status gdca_log_partition(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *x, const int8_t *mask,
                               int32_t flags, const double *betas, int32_t L, int32_t sweep, int32_t K, uint64_t seed, uint64_t stream0,
                               double *out4, double *logw, double *E_end, int8_t *X0, int8_t *Xout, int32_t *accepted, double *thr,
                               int32_t *moves);

/* ---- Boltzmann-machine refinement: fit the Potts model the Metropolis chains draw from ----------------------------------------------
 * The chains sample exp(-beta E) with E(x) = 1/2 (x - Pi)' mJ (x - Pi): read that way (mJ, Pi) IS a Potts model -- couplings the
 * off-diagonal blocks of mJ, fields g - 1/2 diag(mJ), g = mJ Pi.  These entry points fit that model to a family's one- and two-site
 * frequencies by Boltzmann-machine learning: sample, tally, move every parameter by the difference between the model's and the data's
 * frequency, repeat.
 * THE CONTAINER (no new format).  A Potts model in the gauge "the gap's row is zero" is the pair (W, 0) in mJ's layout: W n x n,
 * n = N (q - 1), column-major, full symmetric; its off-diagonal blocks are the couplings in E's sign; W[r, r] = -2 h[r] holds the
 * fields; the entries of a diagonal block off the diagonal are exactly +0.0; Pi is a vector of n zeros.  With Pi = 0 the formulas above
 * reduce to E(x) = sum_{i<j} W[r_i, r_j] + 1/2 sum_i W[r_i, r_i] and V(x; i, c) = sum_{j != i} W[r(i,c), r_j] + 1/2 W[r(i,c), r(i,c)]
 * (g = W 0 = +0.0), so gdca_energies*, gdca_mutation_scan*, gdca_double_mutant*, gdca_greedy_walk*, gdca_sample*, gdca_fn* and
 * gdca_apc* take (W, zeros) AS THEY ARE: that is the whole interface between a learned model and the rest of the library.
 *
 * gdca_potts_from_gaussian_dev: the warm start, W from (mJ, Pi).  Only the lower triangle of mJ is read.  Outside the diagonal blocks
 * W[r, c] = W[c, r] = the bits of mJ[max(r, c), min(r, c)]; inside one, off the diagonal, +0.0; W[r, r] = mJ[r, r] - 2 g[r] (2 g[r]
 * is exact: one subtraction).  g = mJ Pi is the g of the energies and of the mutation scan (the same code), summed in this order: the
 * columns are cut into blocks of 64 (c / 64); inside block o a partial p_o = the products mJ[r, c] Pi[c] (each rounded once, no FMA)
 * added one by one to +0.0 with c ascending -- in r's own block first the columns c <= r, then apart the columns c > r, and the two
 * partials added --; g[r] = the p_o added one by one to +0.0 with o ascending.  Columns beyond n in the last block add +0.0.  W may
 * not alias mJ (GDCA_EINVAL).
 *
 * gdca_bm_update_dev: ONE gradient step on W in place.  For every entry (r, c), in f64, one rounding an operation, no FMA:
 *     d = Pij_m[r, c] - Pij_d[r, c]
 *     m = 2 if r == c, else 0 if r and c belong to the same site, else 1;          g = m d                              (exact)
 *     where m == 1 and lambda != 0:  g = g - lambda W[r, c]                        (one product, one subtraction)
 *     W[r, c] = W[r, c] + eta g                                                    (one product, one addition)
 * Every entry is computed from its own three operands: tallies that are symmetric to the bit (gdca_frequencies*'s and
 * gdca_add_pseudocount*'s are) give both triangles the same bits, and the +0.0 of the diagonal blocks stays +0.0.  This is gradient
 * ascent on the log-likelihood in a gauge without redundant parameters (a concave problem); fields and couplings move at the same
 * rate, the L2 penalty lambda acts on the couplings alone.  The diagonal works through Pij alone (Pij[r, r] = Pi[r] in both tallies,
 * and add_pseudocount keeps that): Pi_d and Pi_m are not read here and may be NULL.  eta > 0 and lambda >= 0, both finite.
 *
 * gdca_bm_readout_dev: the fit in four f64.  Only the lower triangles of Pij_d and Pij_m are read.  With c_x[r, c] = Pij_x[r, c] -
 * Pi_x[r] Pi_x[c] (one rounded product, one subtraction) and P = the entries (r, c) with site(r) > site(c) (T = s^2 N (N - 1) / 2):
 *     out[0] = max_r |Pi_m[r] - Pi_d[r]|;    out[1] = max_P |c_m - c_d|  (one subtraction of the two c, 0 where P is empty);
 *     out[2] = the Pearson correlation of c_m and c_d over P: (T Sab - Sa Sb) / (sqrt(T Saa - Sa Sa) sqrt(T Sbb - Sb Sb)), every
 *              operation rounded once, from the five sums Sa, Sb, Saa, Sab, Sbb over P taken in a fixed order: a column's entries by
 *              256 strided partial sums (partial t: the rows r0 + t, r0 + t + 256, .. ascending, r0 the first row below the column's
 *              diagonal block) folded by a halving tree (t and t + 128, then t and t + 64, ..), the columns' sums the same way.  NaN
 *              where P is empty or a variance is not positive;
 *     out[3] = +0.0 in this form (the loop writes the acceptance rate there).
 * The order is a function of N and q alone, there are no floating-point atomics: the same bits from run to run on any device.
 *
 * gdca_bm_learn_dev: the loop, enqueued without a host round trip per iteration (the device's validity flags are read once, at the
 * end).  W and the chains' states X (N x K int8) are in/out: the chains are persistent.  For t = iter0 .. iter0 + n_iter - 1:
 *     1. the sample stage (gdca_sample_dev's: the scan of X under (W, zeros), then the chains) with stream0 = t K, so every iteration
 *        has streams of its own, n_steps = burn + n_samples stride;
 *     2. X <- every chain's last sample;
 *     3. Pi_m, Pij_m <- gdca_frequencies_dev of the K n_samples samples, unit weights, Meff = K n_samples;
 *     4. the read-out into trace[4 (t - iter0) ..], with out[3] = (the iteration's accepted proposals, summed as integers) /
 *        f64(K n_steps), one division;
 *     5. the update.
 * RULE: a call of n_iter iterations equals, bit for bit in W, X and trace, two calls of a and n_iter - a iterations chained through
 * W, X and iter0 (the second with iter0 + a), and equals the caller doing the steps 1 - 5 with the operator forms.  There is no
 * early stop inside a call: the caller reads trace and calls again.  Xs_last (N x n_samples x K int8, gdca_sample_dev's layout) is
 * optional: the samples of the last iteration.  The workspaces are grow-only buffers of the context (n^2 + 2 n + K n_samples doubles
 * beside the sample stage's and the tally's own).  The bits depend on the context options WALK_TABLE and SAMPLE_CHUNK as little as
 * gdca_sample_dev's do.
 * GDCA_EINVAL, nothing run, W and X untouched: whatever gdca_sample_dev refuses (K, q, flags, beta, burn, stride, n_samples, the
 * table's placement, N); eta <= 0, lambda < 0, either NaN or infinite; n_iter < 1; K n_samples > INT32_MAX;
 * (iter0 + n_iter) K > 2^64 - 1 (the stream numbers would wrap); a null W, Pi_d, Pij_d, X or trace.  A byte of X outside 1..q is
 * reported as gdca_sample_dev reports it (W, X and trace are unspecified then).  All four are new symbols: gdca_stats and gdca_params
 * are unchanged.  There is no fused gdca_run_* form (the inverse is only an initialiser here). */
gdca_status gdca_potts_from_gaussian_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, double *W_dev);
gdca_status gdca_bm_update_dev(gdca_ctx *ctx, double *W_dev, const double *Pi_d_dev, const double *Pij_d_dev, const double *Pi_m_dev,
                               const double *Pij_m_dev, int32_t N, int32_t q, double eta, double lambda);
gdca_status gdca_bm_readout_dev(gdca_ctx *ctx, const double *Pi_d_dev, const double *Pij_d_dev, const double *Pi_m_dev,
                                const double *Pij_m_dev, int32_t N, int32_t q, double *out4_dev);
gdca_status gdca_bm_learn_dev(gdca_ctx *ctx, double *W_dev, const double *Pi_d_dev, const double *Pij_d_dev, int32_t N, int32_t q,
                              int8_t *X_dev, int32_t K, const int8_t *mask_dev, int32_t flags, double beta, uint64_t seed, uint64_t iter0,
                              int32_t n_iter, int32_t burn, int32_t stride, int32_t n_samples, double eta, double lambda, double *trace_dev,
                              int8_t *Xs_last_dev);

/* ---- Pseudo-likelihood fit of the Potts model (plmDCA) --------------------------------------------------------------------------------
 * The container is the Boltzmann machine's: (W, 0) in mJ's layout, the gap the reference state.  With s = q - 1, r(i, c) = i s + c - 1,
 * weights w_k and Meff as gdca_compute_weights* returns them, the objective is
 *     F(W) = (1 / Meff) sum_k w_k sum_i log P(x_ki | x_k,-i ; W),    nll = -F,
 * P(x_i = c | rest) = exp(-V(x; i, c)) / sum_c' exp(-V(x; i, c')) with the mutation stage's site potentials V (GDCA_MUT_POTENTIAL, the
 * gap's V = +0.0).  With p_k[r(i, a)] = P(x_i = a | x_k,-i) the CONDITIONAL TALLIES, in the frequencies' own layout, are
 *     Q[r, c]     = sum_{k : x_k,site(c) = sym(c)} w_k p_k[r]                 Pi_c[r]     = (sum_k w_k p_k[r]) / Meff
 *     Pij_c[r, c] = (Q[r, c] + Q[c, r]) / (2 Meff) outside the diagonal blocks, Pij_c[r, r] = Pi_c[r], +0.0 elsewhere inside one,
 * and dF/dW[r, c] = 2 (Pij_c - Pij_d)[r, c] (the symmetric pair one parameter), dF/dW[r, r] = 1/2 (Pi_c - Pi_d)[r] with (Pi_d, Pij_d)
 * gdca_frequencies*'s of the family.  So gdca_bm_update_dev(W, Pij_d, Pij_c, eta, lambda) IS an ascent step on F - lambda sum_{i<j}
 * |W_ij|^2 (fields at rate eta, couplings at eta / 2 in natural parameters), and gdca_bm_readout_dev(Pi_d, Pij_d, Pi_c, Pij_c) the fit
 * read-out.  eta <= 1 / (N + 2 lambda) keeps nll + lambda sum |W_ij|^2 from rising in exact arithmetic.
 *
 * gdca_plm_conditionals_dev: p (the scan's layout: p[(c - 1) + q (i + N k)], c = 1 .. q, the gap's probability last -- q N M doubles) and
 * nll_k (M) of the M sequences Z (N x M int8) under (W, zeros).  The potentials are gdca_mutation_scan_dev's bits; then per (k, i), f64,
 * one rounding an operation:  m = min_c V_c;  e_c = exp(m - V_c);  Zs = e_1 + .. + e_q added to +0.0 with c ascending;  p_c = e_c / Zs;
 * l_ki = (V[x_ki] - m) + log(Zs);  nll_k = the l_ki added to +0.0 with i ascending BY ONE THREAD.  exp and log are the device library's:
 * their bits are not pinned (the tests hold p and l to an ulp bar).  The largest e_c is 1, so nothing overflows whatever V spans.
 *
 * gdca_plm_tally_dev: (p, Z, w, Meff) -> (Pi_c, Pij_c).  ORDER-FIXED, no floating-point atomics: a = w_k p_k[r] is one rounded product;
 * the sequences are cut into blocks of PLM_CHUNK (context option, default 512); inside a block an entry's terms are added to +0.0 with
 * k ascending (only the sequences that select the entry: the others add nothing); the blocks' partials are added to +0.0 with the block
 * index ascending; Pi_c's sum takes every sequence the same way.  Then one addition of Q and its transpose (it commutes: Pij_c is
 * symmetric to the bit), 2 Meff exact, ONE division an entry.  The order depends on N, q, M and PLM_CHUNK alone: another PLM_CHUNK,
 * other bits.
 *
 * gdca_plm_tallies_dev: the two fused over slabs of sequences (context option PLM_SLAB; a slab is whole blocks, so the bits do not
 * depend on it), p never held beyond a slab.  nll = (sum_k w_k nll_k) / Meff: the rounded products w_k nll_k of k = t, t + 256, .. added
 * to +0.0 ascending into partial t, the 256 partials folded by a halving tree (t and t + 128, t and t + 64, ..), one division.
 *
 * gdca_plm_learn_dev: per iteration t = 0 .. n_iter - 1 it enqueues the tallies; gdca_bm_readout_dev's read-out into trace[4 t ..] with
 * out[3] = nll; gdca_bm_update_dev's step on W.  RULE: n_iter iterations equal a and n_iter - a iterations chained through W, and equal
 * the caller's chain of the operator forms, bit for bit in W and trace, whatever PLM_SLAB.  The weights' range is checked before the
 * first iteration (one round trip a call), the sequences' flags are read once at the end.
 * GDCA_EINVAL, nothing run, every output and W untouched: a null pointer; q outside 2 .. 31; N or M < 1; Meff not positive and finite; a
 * weight outside [0, 1]; eta <= 0, lambda < 0, either NaN or infinite; n_iter < 1; W (p for the tally) aliasing an output.  A byte of Z
 * outside 1 .. q is reported as gdca_mutation_scan_dev reports it (the outputs are unspecified then).  New symbols only: gdca_stats and
 * gdca_params are unchanged. */
gdca_status gdca_plm_conditionals_dev(gdca_ctx *ctx, const double *W_dev, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, double *p_dev,
                                      double *nll_k_dev);
gdca_status gdca_plm_tally_dev(gdca_ctx *ctx, const double *p_dev, const int8_t *Z_dev, const double *w_dev, double Meff, int32_t N, int32_t M,
                               int32_t q, double *Pi_c_dev, double *Pij_c_dev);
gdca_status gdca_plm_tallies_dev(gdca_ctx *ctx, const double *W_dev, const int8_t *Z_dev, const double *w_dev, double Meff, int32_t N,
                                 int32_t M, int32_t q, double *Pi_c_dev, double *Pij_c_dev, double *nll_dev);
gdca_status gdca_plm_learn_dev(gdca_ctx *ctx, double *W_dev, const int8_t *Z_dev, const double *w_dev, double Meff, const double *Pi_d_dev,
                               const double *Pij_d_dev, int32_t N, int32_t M, int32_t q, int32_t n_iter, double eta, double lambda,
                               double *trace_dev);
/* ... with host pointers: upload, the _dev form, download (W in place) */
gdca_status gdca_plm_conditionals(gdca_ctx *ctx, const double *W, const int8_t *Z, int32_t N, int32_t M, int32_t q, double *p, double *nll_k);
gdca_status gdca_plm_tally(gdca_ctx *ctx, const double *p, const int8_t *Z, const double *w, double Meff, int32_t N, int32_t M, int32_t q,
                           double *Pi_c, double *Pij_c);
gdca_status gdca_plm_tallies(gdca_ctx *ctx, const double *W, const int8_t *Z, const double *w, double Meff, int32_t N, int32_t M, int32_t q,
                             double *Pi_c, double *Pij_c, double *nll);
gdca_status gdca_plm_learn(gdca_ctx *ctx, double *W, const int8_t *Z, const double *w, double Meff, const double *Pi_d, const double *Pij_d,
                           int32_t N, int32_t M, int32_t q, int32_t n_iter, double eta, double lambda, double *trace);

/* ---- operator level (host pointers): what the DCAUtils-named wrappers bind -------------- */
/* A host-pointer form on a context with an enqueued run (gdca_run_dev_async, gdca_run_ranked_async, ...) is refused (GDCA_EINVAL)
 * before it touches the context: nothing is uploaded or reallocated, and the enqueued run is unaffected. */
/* compute_theta's all-pairs identity sum (inside compute_weighted_frequencies, :28) */
gdca_status gdca_pair_identity_sum(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, uint64_t *out);
/* theta = min(0.5, 0.38*0.32 / mean pair identity) */
gdca_status gdca_compute_theta(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, double *theta);
/* n_out[k] = 1 + #{l != k : Hamming(k,l) < thresh}  (compute_weights, :28) */
gdca_status gdca_neighbour_counts(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, int32_t thresh,
                                  int32_t *n_out);
/* compute_weights(Z, q, theta): W[M] = 1/n_k, Meff = the sum of the W[k], exact and rounded once (order-independent).
 * theta < 0 selects :auto.  theta_used / thresh may be NULL. */
gdca_status gdca_compute_weights(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, double theta,
                                 double *W, double *Meff, double *theta_used, int32_t *thresh);
/* weighted one-/two-site frequencies (compute_weighted_frequencies' accumulation, :28):
 * Pi[n], Pij[n x n] full symmetric.  Every W[k] must lie in [0, 1] and every byte of Z in 1..q (GDCA_EINVAL). */
gdca_status gdca_frequencies(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, int32_t q,
                             const double *W, double Meff, double *Pi, double *Pij);
/* add_pseudocount(Pi_true, Pij_true, pc, q) (:30) */
gdca_status gdca_add_pseudocount(gdca_ctx *ctx, const double *Pi_true, const double *Pij_true, int32_t N,
                                 int32_t q, double pc, double *Pi, double *Pij);
/* compute_C(Pi, Pij) = Pij - Pi*Pi' (:32, :76) */
gdca_status gdca_covariance(gdca_ctx *ctx, const double *Pi, const double *Pij, int32_t n, double *C);
/* inv(cholesky(C)) (:34): A (n x n, full symmetric) is replaced by its inverse (full
 * symmetric).  *info = 0, or k > 0 when the leading minor of order k is not positive
 * definite (then GDCA_ENOTPD is returned and A is unspecified). */
gdca_status gdca_spd_inverse(gdca_ctx *ctx, double *A, int32_t n, int32_t *info);
/* compute_FN(mJ, q) (:39): S[N x N], diagonal 0 */
gdca_status gdca_fn(gdca_ctx *ctx, const double *mJ, int32_t N, int32_t q, double *S);
/* compute_DI_gauss(mJ, C, q) (:37) */
gdca_status gdca_di(gdca_ctx *ctx, const double *mJ, const double *C, int32_t N, int32_t q, double *S);
/* correct_APC(S) (:42, :78-86), in place */
gdca_status gdca_apc(gdca_ctx *ctx, double *S, int32_t N);

/* energies with host pointers: upload, the _dev form, download (the n x n matrix crosses PCIe: a caller who has just fitted the model
 * uses gdca_run_energies, where only Z, X and E do) */
gdca_status gdca_energies(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                          double *E);
gdca_status gdca_run_energies(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                              const int8_t *X_host, int32_t K, double *E_host, gdca_stats *st);

/* pair energies with host pointers: upload, the _dev form, download */
gdca_status gdca_pair_energies(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, int32_t split, const int8_t *XA,
                               int32_t KA, const int8_t *XB, int32_t KB, int32_t what, double *E);
gdca_status gdca_run_pair_energies(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                   int32_t split, const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, int32_t what,
                                   double *E_host, gdca_stats *st);

/* partner matching with host pointers: upload, the _dev form, download (E_host of gdca_run_partner_match may be NULL: only the
 * matching comes back) */
gdca_status gdca_pair_energies_blocked(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, int32_t split,
                                       const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, const void *offA, const void *offB,
                                       int32_t S, int32_t what, double *E);
gdca_status gdca_assign_blocks(gdca_ctx *ctx, const double *E, const void *offA, const void *offB, int32_t S, int32_t *match, double *gap);
gdca_status gdca_run_partner_match(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                   int32_t split, const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, const void *offA,
                                   const void *offB, int32_t S, int32_t what, double *E_host, int32_t *match_host, double *gap_host,
                                   gdca_stats *st);

/* pair log-odds with host pointers: upload, the _dev form, download (L_host of gdca_run_partner_logodds may be NULL) */
gdca_status gdca_pair_logodds(gdca_ctx *ctx, const double *mJ, const double *mJA, const double *mJB, const double *Pi, int32_t N, int32_t q,
                              int32_t split, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, double I, double *L);
gdca_status gdca_pair_logodds_blocked(gdca_ctx *ctx, const double *mJ, const double *mJA, const double *mJB, const double *Pi, int32_t N,
                                      int32_t q, int32_t split, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, const void *offA,
                                      const void *offB, int32_t S, double I, double *L);
gdca_status gdca_run_pair_logodds(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                  const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, double *L_host, double *EmA_host,
                                  double *EmB_host, double *info, gdca_stats *st);
gdca_status gdca_run_partner_logodds(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                     int32_t split, const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, const void *offA,
                                     const void *offB, int32_t S, double *L_host, int32_t *match_host, double *gap_host, double *info,
                                     gdca_stats *st);

/* iterative partner matching with host pointers: upload, the _dev form, download (gdca_concat_pairs takes the caller's whole Z and
 * touches the requested columns alone; after a failed round gdca_run_partner_ipa still brings back the completed rounds' results) */
gdca_status gdca_select_confident(gdca_ctx *ctx, const int32_t *match, const double *gap, int32_t KA, int32_t n_take, int32_t *sel,
                                  int32_t *n_sel);
gdca_status gdca_concat_pairs(gdca_ctx *ctx, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, int32_t N, int32_t split,
                              const int32_t *selA, const int32_t *selB, int32_t n_sel, int8_t *Z, int32_t col0);
gdca_status gdca_run_partner_ipa(gdca_ctx *ctx, const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, const void *offA,
                                 const void *offB, int32_t S, int32_t N, int32_t q, int32_t split, int32_t what, const gdca_params *p,
                                 const int8_t *Zfix_host, int32_t Mfix, const int32_t *seedA, const int32_t *seedB, int32_t n_seed,
                                 int32_t n_inc, int32_t max_rounds, int32_t *match_host, double *gap_host, int32_t *match_trace_host,
                                 double *gap_trace_host, double *rounds_out, int32_t *rounds_run, gdca_stats *st);

/* mutation scan with host pointers: upload, the _dev form, download */
gdca_status gdca_mutation_scan(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                               int32_t what, double *D);
gdca_status gdca_run_mutation_scan(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                   const int8_t *X_host, int32_t K, int32_t what, double *D_host, gdca_stats *st);

/* double-mutant scan with host pointers: upload, the _dev form, download */
gdca_status gdca_double_mutant_scan(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                                    double *Emin, int32_t *code, double *epi);
gdca_status gdca_double_mutants(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                                const void *muts, int32_t L, double *out);
gdca_status gdca_run_double_mutant_scan(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                        const int8_t *X_host, int32_t K, double *Emin_host, int32_t *code_host, double *epi_host,
                                        gdca_stats *st);
gdca_status gdca_run_double_mutants(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                    const int8_t *X_host, int32_t K, const void *muts_host, int32_t L, double *out_host, gdca_stats *st);

/* greedy walk with host pointers: upload, the _dev form, download */
gdca_status gdca_greedy_walk(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                             const int8_t *mask, int32_t flags, double min_gain, int32_t max_steps, int8_t *Xout, int32_t *steps,
                             double *dE_sum, int32_t *path, double *dE_path, double *V);
gdca_status gdca_run_greedy_walk(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                 const int8_t *X_host, int32_t K, const int8_t *mask, int32_t flags, double min_gain, int32_t max_steps,
                                 int8_t *Xout, int32_t *steps, double *dE_sum, int32_t *path, double *dE_path, double *V, gdca_stats *st);

/* Metropolis chains with host pointers: upload, the _dev form, download */
gdca_status gdca_sample(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                        const int8_t *mask, int32_t flags, double beta, uint64_t seed, uint64_t stream0, int32_t burn, int32_t stride,
                        int32_t n_samples, int8_t *Xs, double *dE_s, int32_t *accepted, double *thr, int32_t *moves, double *V);
gdca_status gdca_run_sample(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                            const int8_t *X_host, int32_t K, const int8_t *mask, int32_t flags, double beta, uint64_t seed,
                            uint64_t stream0, int32_t burn, int32_t stride, int32_t n_samples, int8_t *Xs, double *dE_s, int32_t *accepted,
                            double *thr, int32_t *moves, double *V, gdca_stats *st);

/* Replica-exchange chains with host pointers: upload, the _dev form, download */
gdca_status gdca_sample_tempered(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *Xr,
                                 const int32_t *slot0, int32_t K, int32_t R, const double *betas, const int8_t *mask, int32_t flags,
                                 uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride, int32_t n_samples,
                                 int8_t *Xs, double *E_s, int32_t *accepted, int32_t *swaps, int8_t *Xr_out, int32_t *slot_out, double *thr,
                                 int32_t *moves, double *swap_thr, int32_t *slot_path);
gdca_status gdca_run_sample_tempered(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                     const int8_t *X_host, int32_t K, int32_t R, const double *betas, const int8_t *mask, int32_t flags,
                                     uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride, int32_t n_samples,
                                     int8_t *Xs, double *E_s, int32_t *accepted, int32_t *swaps, int8_t *Xr_out, int32_t *slot_out,
                                     double *thr, int32_t *moves, double *swap_thr, int32_t *slot_path, gdca_stats *st);

/* Boltzmann-machine refinement with host pointers: upload, the _dev form, download (W, X in place) */
gdca_status gdca_potts_from_gaussian(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, double *W);
gdca_status gdca_bm_update(gdca_ctx *ctx, double *W, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int32_t N,
                           int32_t q, double eta, double lambda);
gdca_status gdca_bm_readout(gdca_ctx *ctx, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int32_t N, int32_t q,
                            double *out4);
gdca_status gdca_bm_learn(gdca_ctx *ctx, double *W, const double *Pi_d, const double *Pij_d, int32_t N, int32_t q, int8_t *X, int32_t K,
                          const int8_t *mask, int32_t flags, double beta, uint64_t seed, uint64_t iter0, int32_t n_iter, int32_t burn,
                          int32_t stride, int32_t n_samples, double eta, double lambda, double *trace, int8_t *Xs_last);

/* ---- host-side utilities around the hot path (plain C++, no GPU): the reference's callers of the path -------- */
/* CPUs this process can really use: hardware threads capped by the cgroup CPU quota (a container may see 256 threads and be given
 * 16 CPUs' worth of time; threads beyond the quota are throttled).  What the reader's and the batch driver's thread counts go by. */
int32_t gdca_host_cpus(void);
typedef struct gdca_fasta gdca_fasta;
/* DCAUtils.read_fasta_alignment(filename, max_gap_fraction) (src/GaussDCA.jl:20): parses a FASTA file (plain or
 * gzip), keeps the columns of the first record that are neither '.' nor lowercase, drops sequences with more
 * than max_gap_fraction '-' among them, maps ACDEFGHIKLMNPQRSTVWY -> 1..20, anything else -> 21.
 * open: parse, report N and M;  copy: fill the caller's N x M int8 matrix;  close: free the handle. */
gdca_status gdca_fasta_open(const char *path, double max_gap_fraction, gdca_fasta **out, int32_t *N, int32_t *M);
gdca_status gdca_fasta_copy(const gdca_fasta *h, int8_t *Z);
/* The parsed matrix in place (N x M column-major, valid until gdca_fasta_close; for callers that hand it straight to
 * gdca_run instead of copying it into an array of their own) and its largest symbol, q = maximum(Z) (src/GaussDCA.jl:25). */
const int8_t *gdca_fasta_data(const gdca_fasta *h);
int32_t gdca_fasta_max_symbol(const gdca_fasta *h);
gdca_status gdca_fasta_close(gdca_fasta *h);
/* DCAUtils.remove_duplicate_sequences(Z) (:21-23): first occurrences, order kept.  Z_out may alias Z.
 * keep_idx (optional, M entries): 1-based indices kept. */
gdca_status gdca_remove_duplicates(const int8_t *Z, int32_t N, int32_t M, int8_t *Z_out, int32_t *keep_idx,
                                   int32_t *M_out);
/* compute_ranking(S, min_separation) (:88-99): (i, j, S[j,i]) for j >= i + min_separation, 1-based, stable sort
 * by score descending.  Outputs hold gdca_ranking_length(N, min_separation) entries. */
int64_t gdca_ranking_length(int32_t N, int32_t min_separation);
gdca_status gdca_ranking(const double *S, int32_t N, int32_t min_separation, int32_t *i_out, int32_t *j_out,
                         double *score_out);
/* The same ranking computed on the device from a score matrix in HBM (N x N column-major, N <= 65535; a stable radix sort on the
 * same key: entry for entry the result of gdca_ranking); outputs are host arrays of gdca_ranking_length entries. */
gdca_status gdca_ranking_dev(gdca_ctx *ctx, const double *S_dev, int32_t N, int32_t min_separation, int32_t *i_out,
                             int32_t *j_out, double *score_out);
/* src/GaussDCA.jl:28-44 in one call: gdca_run followed by compute_ranking on the device -- Z (host) in, the ranking (host
 * arrays of gdca_ranking_length(N, min_separation) entries) out; the N x N score matrix never crosses PCIe. */
gdca_status gdca_run_ranked(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                            int32_t min_separation, int32_t *i_out, int32_t *j_out, double *score_out, gdca_stats *st);
/* The same in two halves, for a host thread that keeps two contexts of one GPU busy (gdca_ctx_create_peer): _async uploads Z (the
 * calling thread is held while a pageable Z is staged -- the GPU meanwhile works on what the other context enqueued) and enqueues
 * hot path + ranking without waiting for them; _collect waits and brings the ranking back.  Between the two calls the context
 * accepts nothing else (GDCA_EINVAL), and Z_host may be released as soon as _async has returned. */
gdca_status gdca_run_ranked_async(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                  int32_t min_separation);
gdca_status gdca_run_ranked_collect(gdca_ctx *ctx, int32_t *i_out, int32_t *j_out, double *score_out, gdca_stats *st);
/* K families at once on K contexts of one device (K <= 64; ctxs[0] leads: its options decide the merging, its last_error carries a
 * member's message): uploads, gdca_run_dev_phased -- K front ends, the SPD inverses with the small ones sharing launches of the
 * sweep kernel (options MERGE, MERGE_BLOCKS, ...), K score stages -- and every member's ranking, nothing waited for.  Each member
 * is then collected by itself with gdca_run_ranked_collect, in any order.  What `gdca_cli --batch` runs its small families through. */
gdca_status gdca_run_ranked_phased_async(gdca_ctx *const *ctxs, int32_t K, const int8_t *const *Z_host, const int32_t *N,
                                         const int32_t *M, const int32_t *q, const gdca_params *p, int32_t min_separation);
/* printrank(filename, R) (:67-74): one "%i %i %e" line per entry */
gdca_status gdca_write_rank(const char *path, const int32_t *i, const int32_t *j, const double *score, int64_t len);

/* ---- measurement helpers (bench.py / profiles; not part of the reference surface) ------- */
/* Deterministic "Pfam-like" synthetic family: SplitMix64 streams, integer-threshold draws only, so
 * the same (N, M, q, seed) gives the same bytes everywhere.  Root sequence uniform over 1..q-1; ceil(M/25) cluster
 * centres = root with each site resampled w.p. 1/4; each sequence = a uniformly chosen centre with per-sequence
 * mutation rate from {.02,.05,.1,.2,.3,.5}, then 0-3 gap runs (symbol q) of length U[1, max(2, N/10)].
 * Z is [M][N] (= the N x M column-major matrix).  Needs 2 <= q <= 31. */
gdca_status gdca_synth_family(int32_t N, int32_t M, int32_t q, uint64_t seed, int8_t *Z);
/* Write Z as FASTA (letters of read_fasta_alignment's map, q=21 symbol '-'; headers ">s<k>"); gzip when the path
 * ends in ".gz".  So a reference installation can be fed the same family gdca_synth_family produced. */
gdca_status gdca_write_fasta(const char *path, const int8_t *Z, int32_t N, int32_t M);
/* Dense f64 MFMA issue-rate probe: returns achieved TFLOP/s of a register-resident
 * v_mfma_f64_16x16x4_f64 loop (16 independent accumulators per wave) on every CU: 76-77 on MI355X. */
gdca_status gdca_probe_mfma_f64(gdca_ctx *ctx, int32_t iters, double *tflops);

#ifdef __cplusplus
}
#endif
#endif /* GDCA_H */
