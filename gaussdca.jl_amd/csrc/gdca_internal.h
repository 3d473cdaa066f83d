// Internal declarations shared by the HIP translation units of libgdca.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "gdca.h"
#include "gdca_inverse_outcome.h"

#define GDCA_TILE 128     // tile edge of the SPD-inverse kernels (f64 elements)
#define GDCA_HTILE 128    // sequences per side of a Hamming tile
#define GDCA_MAXQ 31

// The timeline of a fused run: its stage boundaries in stream order.  A boundary is marked by one of two clocks -- a HIP event of the
// context, or a 100 MHz device time stamp in gdca_dev_scalars::stamp -- and both are indexed by this enum (gdca_api.hip: mark, elapsed).
enum gdca_boundary {
    T_NONE = -1,
    T_BEGIN, T_THETA, T_WEIGHTS,
    T_TALLY_BEGIN, T_TALLY_END,                              // around k_pair_tally of the covariance's first build (gdca_stats.ms_pair_tally)
    T_COV,
    T_INV_BEGIN, T_SWEEP_BEGIN, T_SWEEP_END, T_INV_END,      // the run's turn on the MFMA pipe (behind any pipeline gate), and the sweep kernel alone in it
    T_SCORE_BEGIN, T_FN_BEGIN, T_FN_END, T_END,              // the score stage, and k_fn alone in it (gdca_stats.ms_fn)
    T_COUNT
};

// Scalars that live in HBM so the whole pipeline can be enqueued without a host round trip.
struct gdca_dev_scalars {
    double theta;
    double Meff;
    unsigned long long pair_sum;
    int thresh;
    int info;
    int bad_symbol;  // what the kernels found wrong with the caller's data, one bit a kind: the GDCA_BAD_* of gdca_inverse_outcome.h (GDCA_EINVAL)
    int di_noconv;   // number of site pairs whose tridiagonal QL iteration did not converge (DI score)
    int ham_mode;    // all-pairs Hamming kernel chosen for this family: 0 = exact distances, 1 = three-plane lower bound + refinement, 2 = the consensus
                     // lower bound on the fp4 matrix pipe + refinement (k_hamming_fp4.hip)
    int ham_cand;    // candidate pairs (bound below the threshold) in the sampled tiles of k_hamming_probe
    unsigned long long ham_ncand;  // pairs the bound form has put (or tried to put) into its candidate list: beyond the list's capacity the exact form counts
    unsigned long long sweep_cycles, sweep_ticks;  // k_sweep, summed over its workgroups: shader-clock cycles (s_memtime) and 100 MHz ticks they ran for
    double inv_norm1;  // ||inverse||_1 as the sweep left it (0: not measured)
    double ns_resid;     // max |I - X0 C| seen by the Newton-Schulz step (0: no step)
    double mat_norm1;  // ||C||_1: measured on the covariance before the sweep where the cheap bound leaves the question open (fused path), or on the
                       // caller's matrix (operator-level inverse); 0: not measured
    double pi_max;     // max over the n single-site frequencies with pseudocount (k_pi_finalize): ||C||_1 <= 2 N pi_max
    // device time stamps (100 MHz wall clock) of a run whose kernels were issued as batched grids (gdca_run_dev_phased: no HIP events
    // between them -- an event per member and stage was most of the host's work for a batch)
    unsigned long long stamp[T_COUNT];
    int ham_cand2;   // pairs of the sampled tiles the consensus form would list (D1 < thresh)
    int ham_cut;     // word at which the three-plane bound form goes from all pairs of a tile to the list of those still below the threshold
                     // (k_hamming_decide; >= NW: never)
    unsigned ham_alive[64];  // k_hamming's probe: pairs of the sampled tiles still below the threshold after w + 1 words (HAM_ALIVE_SLOTS)
    double logdet;   // log det of the matrix the last inverse was taken of: the sum of the logarithms of its pivots (k_logdet); NaN where info != 0
};

// Tuning switches of one context (gdca_ctx_set_option): initialised from the GDCA_* environment variables when the context is
// created, never read from the environment afterwards -- two contexts of one process may differ, and a switch changed through
// gdca_ctx_set_option takes effect at the next call on that context.  -1 = "the measured rule" where a rule exists.
struct gdca_tuning {
    int group;              // GDCA_GROUP: pivot blocks per group of the sweep, 1..4
    int ramp;               // GDCA_RAMP: 0 = uniform groups, the remainder last
    int ragged;             // GDCA_RAGGED: 0 = sweep the matrix padded to 128 instead of 16
    int rem_tail;           // GDCA_REM_TAIL: remainder tiles of update p listed after panel(p+1)
    int panel_halves;       // GDCA_PANEL_HALVES: 1 = two 128 x 64 panel items per pivot block and row, 0 = one 128 x 128
    int slab;               // GDCA_SLAB: 0 = panel and tile items between single blocks instead of the fused row slabs
    int ring;               // GDCA_RING: panel / Pg slots between single blocks (2..8)
    int mcus;               // GDCA_MCUS: compute units elected for the pivot chain (1..16)
    int mcu_solo;           // GDCA_MCU_SOLO: 1 = one chain worker per elected compute unit (its second workgroup leaves; MCUS then counts up to 32), 0 = two, -1 = the measured rule (groups of two and three)
    int sweep_debug;        // GDCA_SWEEP_DEBUG (tests): bit 0 = XCC 0 stays out of the election, bit 1 = nobody is elected, bit 5 = the watchdog ends the first attempt of every inverse
    long sweep_timeout_ms;  // GDCA_SWEEP_TIMEOUT_MS: bound of one dependency wait; 0 = scaled with the problem (>= 4 s)
    int sweep_retries;      // GDCA_SWEEP_RETRIES: attempts an inverse gets after its launch was ended by the watchdog (default 2; 0 = none: GDCA_EHIP at once)
    int tally_tj;           // GDCA_TALLY_TJ: 32 = the wide pair-tally form
    int tally_skip;         // GDCA_TALLY_SKIP: 1 = the pair tally skips each column's most frequent symbol and recovers its row (default), 0 = the full loop
    int hamming_mode;       // GDCA_HAMMING_MODE: -1 = probe, 0 = full (exact five-plane distances), 1 = bound (three planes + refinement), 2 = mfma (the consensus plane on the fp4 matrix pipe + refinement)
    int ham_cut;            // GDCA_HAM_CUT (tests, measurements): 0 = the bound form's cut word from the probe (default), k >= 1 = switch at word k (k >= NW: never)
    int force_fallback;     // GDCA_FORCE_FALLBACK: 1 = the independent byte-compare Hamming kernel
    int merge;              // GDCA_MERGE: families one merged sweep launch may carry in gdca_run_dev_phased (1 = never merge)
    int merge_blocks;       // GDCA_MERGE_BLOCKS: largest member of a merged launch, in 128-blocks
    int merge_mcus;         // GDCA_MERGE_MCUS: chain compute units per member of a merged launch
    int merge_group;        // GDCA_MERGE_GROUP: pivot blocks per group of a member of a merged launch, 1..4
    int merge_tiles;        // GDCA_MERGE_TILES: a merged launch is closed once its members hold this many tiles per update step
    int phased_fronts;      // GDCA_PHASED_FRONTS: 1 = the front ends of a phase batch run side by side on the members' own streams (default), 0 = one after the other on the leader's
    int phased_grids;       // GDCA_PHASED_GRIDS: the kernels of a phase batch's front ends and score stages go out as ONE grid per kernel kind carrying all members of a group: 1 .. 8 = that many groups of members side by side (front ends; the score stages are always one group), -1 = by the batch's work (default: one group for small families, four for big ones), 0 = one launch per member and kernel
    int phased_streams;     // GDCA_PHASED_STREAMS: streams the side-by-side front ends and score stages of a phase batch are spread over (the first members' own; default 4 = the hardware queues)
    int refine;             // GDCA_REFINE: -1 = one Newton-Schulz step where the inverse looks ill-conditioned (auto), 0 = never, 1 = always
    double refine_cond;     // GDCA_REFINE_COND: the threshold of auto: the a-priori bound of cond_2(C) first, beyond it kappa_1 = ||C||_1 ||X||_1
    int cholesky;           // GDCA_CHOLESKY: the blocked dpotrf + dpotri fallback: 0 = never, 1 = where the sweep gave up (default), 2 = always
    int energy_chunk;       // GDCA_ENERGY_CHUNK: sequences one launch of the energy gather kernel takes; 0 = as many as keep its partials within ~256 MB
    int pair_chunk;         // GDCA_PAIR_CHUNK: sequences of protein A one launch of the pair-energy fold / gather kernels takes; 0 = as many as keep their folded rows within ~256 MB (the rule), a smaller count is taken as given, a larger one is cut to the rule
    int epi_generic;        // GDCA_EPI_GENERIC (tests, measurements): 1 = the double-mutant scan runs its generic instance (s at run time) at s = 20 too
    int walk_table;         // GDCA_WALK_TABLE: where the greedy walk keeps a sequence's table of site potentials: 0 = in LDS where it fits, else in HBM (auto, default), 1 = LDS (a table that does not fit: GDCA_EINVAL), 2 = HBM; the same bits wherever it is (the Metropolis chains share it)
    int sample_chunk;       // GDCA_SAMPLE_CHUNK: proposals one launch of the Metropolis kernel takes; 0 = GDCA_SAMPLE_CHUNK_RULE; the same bits whatever it is
    int plm_chunk;          // GDCA_PLM_CHUNK: sequences a block of the pseudo-likelihood tally sums in one go (k_plm.hip); 0 = GDCA_PLM_CHUNK_RULE; it fixes the order of the sums: another value, other bits
    int plm_slab;           // GDCA_PLM_SLAB: sequences whose conditionals are held at a time (rounded up to whole blocks); 0 = as many as keep the table within ~256 MB; the same bits whatever it is
    char sweep_trace[256];  // GDCA_SWEEP_TRACE: file the in-kernel trace of the next inverse is written to ("" = off)
};
void gdca_tuning_from_env(gdca_tuning *t);
// key: the variable's name with or without the GDCA_ prefix, any case.  false: unknown key or unusable value.
bool gdca_tuning_set(gdca_tuning *t, const char *key, const char *value);

// ---- k_theta.hip -------------------------------------------------------------------------
// Z [M][N] (any alignment) -> Zt [N][M] (Z transposed) and Zc [ceil(N/TJ)][M][TJ] (zero padded; 16-byte aligned), TJ = gdca_tally_tj(q)
void gdca_launch_relayout(hipStream_t s, const int8_t *Z, int8_t *Zt, int8_t *Zc, int N, int M, int TJ);
// cnt: gdca_column_hist_bytes(N, M) bytes: uint32 [N][32], the counts (every one written: nothing to zero), then the kernel's
// per-chunk partial counts
size_t gdca_column_hist_bytes(int N, int M);
void gdca_launch_column_hist(hipStream_t s, const int8_t *Z, uint32_t *cnt, int N, int M);
// theta_in < 0: theta = :auto from cnt; else theta = theta_in.  Writes theta, thresh, pair_sum.
void gdca_launch_theta_finalize(hipStream_t s, const uint32_t *cnt, int N, int M, double theta_in,
                                gdca_dev_scalars *sc);
// sets sc->thresh directly (operator-level neighbour counts with a caller-given threshold)
void gdca_launch_set_thresh(hipStream_t s, gdca_dev_scalars *sc, int thresh);

// ---- k_hamming.hip -----------------------------------------------------------------------
// bit-plane image: uint32 [Mt][5][NW][128], Mt = ceil(M/128), NW = ceil(N/32)
size_t gdca_bitplane_bytes(int N, int M);
// q: largest legal symbol (bytes outside 1..q set sc->bad_symbol)
void gdca_launch_bitplane_pack(hipStream_t s, const int8_t *Z, uint32_t *Zb, int N, int M, int q,
                               gdca_dev_scalars *sc);
// cnt: int32 [Mt*128], zeroed by the caller; adds #{l != k: d(k,l) < sc->thresh}
// force: -1 = decide per family from a sample of tiles, 0 = the exact form, 1 = the lower bound with refinement
// cut: 0 = the bound form's cut word from the sample as well, k >= 1 = at word k (k >= NW: never)
size_t gdca_hamming_cand_cap(int M);  // pairs the bound forms' candidate list holds (8 bytes each)
// ---- k_hamming_fp4.hip: the consensus lower bound on the fp4 matrix pipe (sc->ham_mode == 2) ----
size_t gdca_fp4_image_bytes(int N, int M);  // the image and sigma
// hist: the column histogram [N][32] (gdca_launch_column_hist), already enqueued
void gdca_launch_hamming_fp4_image(hipStream_t s, const int8_t *Z, const uint32_t *hist, void *img, int N, int M);
void gdca_launch_hamming_fp4_probe(hipStream_t s, const void *img, int N, int M, int nprobe, gdca_dev_scalars *sc);
void gdca_launch_hamming_fp4(hipStream_t s, const void *img, int N, int M, gdca_dev_scalars *sc, void *cand_list, unsigned cap);
void gdca_launch_hamming(hipStream_t s, const uint32_t *Zb, const int8_t *Z, int32_t *cnt, int N, int M, gdca_dev_scalars *sc, int force,
                         void *cand_list, void *fp4_img, int cut);
// the same counts by an independent plain byte-compare kernel straight from Z (GDCA_FORCE_FALLBACK; overwrites cnt[0..M-1])
void gdca_launch_hamming_fallback(hipStream_t s, const int8_t *Z, int32_t *cnt, int N, int M, const gdca_dev_scalars *sc);
// n_out[k] = 1 + cnt[k]; W[k] = 1/n_k; Wfix[k] = rint(W[k] * 2^fix_shift)
void gdca_launch_weights(hipStream_t s, const int32_t *cnt, int M, int fix_shift, int32_t *n_out, double *W,
                         unsigned long long *Wfix);
// Meff = the exact sum of the weights, rounded once (one workgroup; order-independent)
void gdca_launch_meff(hipStream_t s, const double *W, int M, gdca_dev_scalars *sc);
// Wfix from caller-given W (operator-level gdca_frequencies)
void gdca_launch_fix_weights(hipStream_t s, const double *W, int M, int fix_shift, unsigned long long *Wfix,
                             gdca_dev_scalars *sc);
int gdca_fix_shift(int M);

// ---- k_tally.hip -------------------------------------------------------------------------
// Pifix: u64 [N][32], every entry written: sum_k Wfix[k] [Z[i,k] & 31 == z] at [i][z] (bytes outside 1..q raise GDCA_BAD_ALIGNMENT in sc->bad_symbol).
// Zt: Z transposed (N rows of M; 4-byte aligned, 3 bytes of slack behind it).  keep != nullptr (TALLY_SKIP): also keep (uint32
// [N][M]; per column i: keep_n[i] entries (k << 5) | Z[i,k], ascending k, every sequence whose Z[i,k] is a legal symbol other than
// sigma[i] = the argmax of Pifix[i][1..q], ties to the smallest), keep_n and sigma
void gdca_launch_pi_keep(hipStream_t s, const int8_t *Zt, const unsigned long long *Wfix, unsigned long long *Pifix, uint32_t *keep,
                         int *keep_n, uint8_t *sigma, int N, int M, int q, gdca_dev_scalars *sc);
// Pi_true[i*s+a] = Pifix * 2^-shift / Meff;  Pi_pc = (1-pc) Pi_true + pc/q
void gdca_launch_pi_finalize(hipStream_t s, const unsigned long long *Pifix, int N, int q, int fix_shift,
                             const double *Meff_dev, double pc, double *Pi_true, double *Pi_pc, double *pi_max = nullptr);
// ||C||_1 of the covariance at C (full symmetric, ld) into sc->mat_norm1 -- only where 2 N pi_max q^2 / pc, the bound of cond(C) that
// costs nothing, exceeds cond_limit (or `always`): otherwise every workgroup leaves at once
void gdca_launch_cov_norm1(hipStream_t s, const double *C, size_t ld, int N, int q, double pc, double cond_limit, gdca_dev_scalars *sc,
                           int always);
// Pair tallies.  mode 0: out = Pij_true (full symmetric, ld);  mode 1: out = C =
// add_pseudocount + compute_C fused (full symmetric, ld).  Pi_pc used by mode 1 only.
// Zc: the alignment regrouped as [ceil(N/TJ)][M][TJ] (gdca_launch_relayout), TJ = gdca_tally_tj(q).
int gdca_tally_tj(int q, int tj_wanted);
// TALLY_SKIP where the [q][q][TJ] histograms fit as many workgroups per CU as the full loop's (and M <= 2^27)
bool gdca_tally_skip(int q, int TJ, int skip_wanted, int M);
// keep == nullptr: the full loop over all M sequences; else keep / keep_n / sigma of gdca_launch_pi_keep and Pifix (the SKIP form)
void gdca_launch_pair_tally(hipStream_t s, const int8_t *Zc, const int8_t *Zt, const unsigned long long *Wfix,
                            int N, int M, int q, int fix_shift, const double *Meff_dev, double pc,
                            const double *Pi_pc, int mode, double *out, size_t ld, int TJ, const uint32_t *keep = nullptr,
                            const int *keep_n = nullptr, const uint8_t *sigma = nullptr, const unsigned long long *Pifix = nullptr);
// out (ld) = the covariance of pseudocount pc built from stored tallies: Pij (n x n, ld = n, mode 0's output) and that pc's Pi_pc --
// bit for bit what mode 1 writes for pc (both triangles; the padding is the caller's: gdca_launch_pad_identity).  ldp != 0: Pij and
// Pi_pc point at the first element of a principal block of N whole sites inside a Pij of leading dimension ldp (0: ldp = n)
void gdca_launch_cov_from_pij(hipStream_t s, const double *Pij, const double *Pi_pc, int N, int q, double pc, double *out, size_t ld,
                              size_t ldp = 0);

// ---- k_elementwise.hip ---------------------------------------------------------------------
void gdca_launch_add_pseudocount(hipStream_t s, const double *Pi_true, const double *Pij_true, int N, int q,
                                 double pc, double *Pi, double *Pij);
void gdca_launch_covariance(hipStream_t s, const double *Pi, const double *Pij, int n, double *C);
// A[n_pad x n_pad] (ld = n_pad): rows/cols >= n become identity
void gdca_launch_pad_identity(hipStream_t s, double *A, int n, int n_pad);
// copy a dense n x n (ld_src) into the padded buffer (ld_dst) / back, with optional negate+mirror
void gdca_launch_copy_in(hipStream_t s, const double *src, int n, double *dst, int n_pad);
// same with the real block negated (mJ -> the "-mJ" image the score kernels read)
void gdca_launch_copy_in_neg(hipStream_t s, const double *src, int n, double *dst, int n_pad);
// dst (n x n, ld n) = full symmetric  -lower(A)  (A holds -inverse in its lower triangle)
void gdca_launch_copy_out_neg_sym(hipStream_t s, const double *A, int n_pad, double *dst, int n);
// *host_mapped (pinned host memory, the device's address of it) = *sc, system-scope visible when the kernel has completed
void gdca_launch_publish_scalars(hipStream_t s, const gdca_dev_scalars *sc, gdca_dev_scalars *host_mapped);
// D[i] (s x s, packed) = diagonal block i of C (ld)
void gdca_launch_save_diag_blocks(hipStream_t s, const double *C, size_t ld, int N, int sdim, double *D);

// ---- k_inverse.hip -------------------------------------------------------------------------
struct gdca_inverse_ws {
    double *G[8];      // n_pad x 128 panels: [4 (p & 1) + w] = column block w of pivot group p (double-buffered by group parity)
    double *H[8];      // n_pad x 128 panels, -G * Pg
    double *P;         // 128 x 128 inverse of one pivot block
    double *piv;       // n_pad pivots of the elimination, row by row (the sweep's side output; the Cholesky fallback writes its L_ii^2 there)
    double *Sg[2];     // 512 x 512 dense scratch copies of a group's diagonal super-block (ping-pong)
    double *Pg[2];     // 512 x 512: inverse of a group's diagonal super-block, by group parity
    unsigned *flags;   // dependency flags of the sweep (zeroed per inverse by the launcher)
    size_t flags_bytes;
    int *item0_host;   // pinned: the sweep's item table -- three tables of ng + 1 entries (gdca_sweep_schedule.h: item0, mitem0, gs), room for gdca_sweep::table_ints_max(n_pad / 128)
    const int *item0_host_dev;  // item0_host as the device addresses it (nullptr: the table goes through hipMemcpyAsync)
    int *item0_dev;
    int update_cus;    // compute units of the device
};
// One inverse: in place on A (n_pad x n_pad, ld = n_pad, lower triangle + full diagonal tiles authoritative): A <- -inverse(A) by
// the block symmetric sweep.  sc->info gets the 1-based index of the first non-positive pivot, if any (GDCA_INFO_WATCHDOG: the kernel's
// watchdog abandoned a dependency wait).
struct gdca_inverse_job {
    double *A;
    int n_pad, n_real;
    gdca_inverse_ws ws;
    gdca_dev_scalars *sc;
    const gdca_tuning *tune;
    bool doomed;  // tests (option SWEEP_DEBUG bit 5): this launch's watchdog fires at its first unsatisfied wait
};
size_t gdca_inverse_flag_bytes(int n_pad);
// ONE persistent launch on stream s; sweep_begin / sweep_end (each may be null) are recorded around the sweep kernel, behind k_sweep_prep.
void gdca_launch_spd_inverse(hipStream_t s, const gdca_inverse_job &job, hipEvent_t sweep_begin, hipEvent_t sweep_end, double *upd_flops);
// K <= gdca_inverse_max_merge() independent inverses (single-block schedules: small matrices) carried by ONE persistent launch;
// every member's arithmetic is that of a launch of its own.  upd_flops: K entries.
int gdca_inverse_max_merge(void);
void gdca_launch_spd_inverse_merged(hipStream_t s, const gdca_inverse_job *jobs, int K, hipEvent_t sweep_begin, hipEvent_t sweep_end,
                                    double *upd_flops);
// ---- k_rank.hip --------------------------------------------------------------------------
// compute_ranking (src/GaussDCA.jl:88-99) of S_dev (N x N column-major): `len` = gdca_ranking_length(N, sep) > 0 entries, sorted,
// left in three arrays inside the workspace `ws` (gdca_ranking_ws_bytes(len) bytes)
size_t gdca_ranking_ws_bytes(long long len);
void gdca_launch_ranking(hipStream_t s, const double *S_dev, int N, int sep, long long len, void *ws, int32_t **ii, int32_t **jj, double **sc);
// the 64-bit key of the ranking's order (the host form's, gdca_host.cpp): ascending keys = descending scores under isless, NaN first,
// 0.0 before -0.0
__device__ __forceinline__ uint64_t gdca_rank_key(double x)
{
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    uint64_t asc = (u >> 63) ? ~u : (u | 0x8000000000000000ull);  // ascending in isless order: -0.0 < 0.0
    if (x != x) asc = ~0ull;                                        // every NaN greatest, all equal
    return ~asc;                                                    // descending
}
// The ranking's eight stable radix passes on given keys and values: n entries in key[0] / val[0], sorted ascending by key into key[0] /
// val[0] again (equal keys keep their order); key[1] / val[1]: as large; hist: gdca_sort_hist_words(n) words
size_t gdca_sort_hist_words(size_t n);
void gdca_launch_sort_pairs(hipStream_t s, uint64_t *const key[2], uint32_t *const val[2], uint32_t *hist, size_t n);
void gdca_launch_probe_mfma_f64(hipStream_t s, double *out, int iters, int blocks);
// The reference's own way (dpotrf + dpotri) as a fallback for matrices the sweep cannot handle: C2 (n_pad x n_pad, identity
// padding; overwritten by its Cholesky factor), U and Tm: n_pad x n_pad workspaces, Wd: (n_pad / 128) tiles of 128 x 128; Aout
// receives -inverse in its lower block triangle (the sweep's storage); sc->info = dpotrf's index of a non-positive pivot
// piv: n_pad doubles, L_ii^2 (the pivots: gdca_inverse_ws::piv)
void gdca_launch_cholesky_inverse(hipStream_t s, double *C2, double *U, double *Tm, double *Wd, double *Aout, int n_pad, int n_real,
                                  gdca_dev_scalars *sc, double *piv);
// *out = ||X||_1 of the symmetric matrix whose lower block triangle is A (= -X, the sweep's storage; first n rows / columns);
// colsum_ws: n_pad doubles
void gdca_launch_inverse_norm1(hipStream_t s, const double *A, int n_pad, int n, double *colsum_ws, double *out);
// *out = max_i |A(i, i)|, i < n
// *out = ||C||_1 of a plain n x n matrix
void gdca_launch_matrix_norm1(hipStream_t s, const double *C, size_t ld, int n, double *colsum_ws, double *out);
// one Newton-Schulz step on the sweep's result: A (-X0 lower block triangle -> -X1), C2 = the matrix that was inverted (full
// symmetric, n_pad x n_pad, identity padding), B0 and Rt: n_pad x n_pad workspaces
// *resid (optional): max |I - X0 C|, the residual the step squares -- below one or the step cannot have converged
void gdca_launch_newton_schulz(hipStream_t s, double *A, const double *C2, double *B0, double *Rt, int n_pad, double *resid);

// ---- k_logdet.hip --------------------------------------------------------------------------
// sc->logdet = sum_{i < n_real} log(piv[i]) in a fixed order (quiet NaN where sc->info != 0), behind the inverse on its stream
void gdca_launch_logdet(hipStream_t s, const double *piv, int n_real, gdca_dev_scalars *sc);
// L[k] <- -(L[k] + c), k < K: energies into log-likelihoods
void gdca_launch_loglik(hipStream_t s, double *L, int K, double c);

// ---- k_score.hip ---------------------------------------------------------------------------
// S (N x N) from the lower triangle of A = -mJ (ld).  Diagonal 0.
void gdca_launch_fn(hipStream_t s, const double *A, size_t ld, int N, int sdim, double *S, int ncu = 0);
// Ld[i] = chol(D[i]) lower, packed s x s
void gdca_launch_diag_chol(hipStream_t s, const double *D, int N, int sdim, double *Ld);
// Tws: workspace of gdca_di_ws_bytes(N, sdim) bytes (tridiagonals of all site pairs)
size_t gdca_di_ws_bytes(int N, int sdim);
void gdca_launch_di(hipStream_t s, const double *A, size_t ld, const double *Ld, int N, int sdim, double *S,
                    double *Tws, gdca_dev_scalars *sc);
void gdca_launch_apc(hipStream_t s, double *S, int N, double *rowsum_ws);

// ---- the model read-outs (k_energy.hip, k_pair_energy.hip, k_mutation.hip) ------------------------------------------------------------
// The fitted model as the read-outs see it: mJ (sign +1) or -mJ (sign -1) in the element-wise lower triangle of A -- element (row,
// col), row >= col, at A[col * ld + row] -- and Pi, the n = N (q - 1) single-site frequencies with pseudocount.  Made in two places
// (gdca_api.hip): from the sweep's storage of a fused run and from an operator's mJ_dev / Pi_dev.
struct gdca_model {
    const double *A;
    size_t ld;
    double sign;
    const double *Pi;
    int N, q;
};

// ---- k_energy.hip: E(x) = 1/2 (x - Pi)' mJ (x - Pi) of K sequences ---------------------------------------------------------------
int gdca_energy_blocks(int Ns);       // site blocks (of four sites = one packed dword) of Ns sites
int gdca_energy_gblocks(int n);       // 64-blocks of the g pass
int gdca_energy_chunk(int N, int K, int wanted);  // sequences one launch of the gather kernel takes (wanted > 0: that many)
// Xg: uint32 [gdca_energy_blocks(Ns)][K] from the Ns sites X points at (sequence k: X + k * stride; whole sequences: stride = Ns = N);
// bytes outside 1..q raise GDCA_BAD_SEQUENCE in sc->bad_symbol (and count as gaps)
void gdca_launch_energy_pack(hipStream_t s, const int8_t *X, size_t stride, int Ns, int K, int q, uint32_t *Xg, gdca_dev_scalars *sc);
// g = mJ Pi (n entries) and c0 = Pi' g from the element-wise lower triangle of A (ld; sign -1: A holds -mJ, the sweep's storage);
// part: nb x (nb * 64) doubles, nb = gdca_energy_gblocks(n)
void gdca_launch_energy_g(hipStream_t s, const double *A, size_t ld, double sign, int n, const double *Pi, double *part, double *g,
                          double *c0);
// E[k0 .. k0 + Kc - 1]; part: gdca_energy_blocks(N) x Kc doubles.  An error (here and below): the dynamic LDS limit could not be raised
// for a kernel's tile; that kernel was not launched
hipError_t gdca_launch_energy_rows(hipStream_t s, const double *A, size_t ld, double sign, const double *g, const double *c0,
                                   const uint32_t *Xg, int N, int sdim, int K, int k0, int Kc, double *part, double *E, int ncu);

// ---- k_pair_energy.hip: E(a (+) b) of K_A x K_B pairings across a split alignment -------------------------------------------------------
int gdca_pair_chunk(int nB, int KA, int wanted);    // sequences a one launch of the fold / gather kernels takes (wanted > 0: that many)
// Xp (N x (KA + KB)): a (+) gaps for the KA sequences of XA (split sites each), then gaps (+) b for the KB of XB (N - split sites each)
void gdca_launch_pair_pad(hipStream_t s, const int8_t *XA, size_t strideA, const int8_t *XB, size_t strideB, int N, int split, int KA, int KB,
                          int q, int8_t *Xp);
// What carries a pair energy on to the log-odds of the pairing against the two marginal models (include/gdca.h, pair log-odds): the
// marginal models' energies of the KA sequences a and of the KB sequences b (device), and I = -1/2 (log det C - log det C_AA - log det C_BB)
struct gdca_logodds_terms {
    const double *EmA, *EmB;
    double I;
};
// E[a + KA * b], a0 <= a < a0 + Ac, all b, from the block rows >= split * sdim, columns < split * sdim of A (ld; sign -1: A holds -mJ);
// XAg / XBg: the halves packed by gdca_launch_energy_pack; T: Ac x (N - split) * sdim doubles.  EAB (KA + KB marginal energies) and c0:
// the energy; EAB == nullptr: the coupling R alone.  lo != nullptr (with EAB): E receives ((EmA[a] + EmB[b]) - energy) + I instead
hipError_t gdca_launch_pair_chunk(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *XAg, const uint32_t *XBg, int N,
                                  int split, int sdim, int KA, int KB, int a0, int Ac, double *T, const double *EAB, const double *c0, double *E,
                                  int ncu, const gdca_logodds_terms *lo = nullptr);
// The pairings inside the species of species-sorted sequences (include/gdca.h, partner matching).  The work list: 4 int32 an item
// (species, first a, first b, na | nb << 8), a ascending, no group of a across a multiple of Ac; first[c] = the first item of chunk c
// (one entry more than chunks).  offA / offB: S + 1 valid offsets
void gdca_pair_block_items(const int32_t *offA, const int32_t *offB, int S, int Ac, std::vector<int32_t> &items, std::vector<long long> &first);
// ... and the blocks of the packed E those items of one chunk cover (items, eoff [S + 1], offA, offB [S + 1]: device); the fold and every
// other argument as gdca_launch_pair_chunk, every entry bit for bit its
hipError_t gdca_launch_pair_chunk_blocked(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *XAg, const uint32_t *XBg, int N,
                                          int split, int sdim, int KA, int KB, int a0, int Ac, double *T, const double *EAB, const double *c0,
                                          double *E, const int32_t *items, long long nitems, const long long *eoff, const int32_t *offA,
                                          const int32_t *offB, int ncu, const gdca_logodds_terms *lo = nullptr);
// dst[i] = -src[i], i < len (the assignment on log-odds minimises -L)
void gdca_launch_negate(hipStream_t s, const double *src, double *dst, size_t len);

// ---- k_assign.hip: the minimum-cost assignment inside every block of a blocked cost matrix -------------------------------------------------
// match[KA] / gap[KA] (gap may be nullptr) of the S species (eoff, offA, offB: device, S + 1 entries each); kmax = the largest kA_s or
// kB_s (<= GDCA_ASSIGN_MAX)
hipError_t gdca_launch_assign_blocks(hipStream_t s, const double *E, const long long *eoff, const int32_t *offA, const int32_t *offB, int S,
                                     int kmax, int32_t *match, double *gap);

// ---- k_ipa.hip: the glue between two rounds of iterative partner matching ---------------------------------------------------------------
// what a round hands to the host (device record; every field written by a kernel, nothing accumulated)
struct gdca_ipa_counts {
    double cost;     // sum over the candidates in ascending a of E[a, match[a]] (k_ipa_round)
    int n_changed;   // a whose match differs from the round before; without a round before: the candidates (k_ipa_round)
    int ncand;       // a with match[a] >= 0 (k_ipa_compact)
    int n_sel;       // the selected (k_ipa_compact)
    int pad_;
};
// The selection (include/gdca.h, gdca_select_confident_dev): sel[KA] = the first min(n_take, candidates) candidates by gap descending (the
// ranking's order, ties in ascending a), in ascending a, then -1; out->ncand, out->n_sel.  ws: gdca_ipa_select_ws_bytes(KA) bytes
size_t gdca_ipa_select_ws_bytes(int KA);
void gdca_launch_ipa_select(hipStream_t s, const int32_t *match, const double *gap, int KA, int n_take, void *ws, int32_t *sel, gdca_ipa_counts *out);
// Columns col0 .. col0 + n_sel - 1 of Z (N rows): XA[:, selA[t]] over XB[:, b], b = viaB ? viaB[selA[t]] : selB[t]; an index outside its
// pool: GDCA_BAD_INDEX in sc->bad_symbol, that column left alone
void gdca_launch_ipa_concat(hipStream_t s, const int8_t *XA, int KA, const int8_t *XB, int KB, int N, int split, const int32_t *selA,
                            const int32_t *selB, const int32_t *viaB, int n_sel, int8_t *Z, size_t col0, gdca_dev_scalars *sc);
// out->cost, out->n_changed of a round's match against the packed blocks E (eoff, offA, offB: the species table; spA[a]: a's species;
// prev: the match of the round before, or nullptr)
void gdca_launch_ipa_round(hipStream_t s, const double *E, const long long *eoff, const int32_t *offA, const int32_t *offB, const int32_t *spA,
                           const int32_t *match, const int32_t *prev, int KA, gdca_ipa_counts *out);
// a completed round's match / gap (KA entries) into prev, match_out and -- each may be nullptr -- gap_out, match_row, gap_row
void gdca_launch_ipa_publish(hipStream_t s, const int32_t *match, const double *gap, int KA, int32_t *prev, int32_t *match_out, double *gap_out,
                             int32_t *match_row, double *gap_row);

// ---- k_mutation.hip: V(x; i, c) / dE(x; i, b) of every single substitution of K sequences ------------------------------------------------
// D[(b - 1) + q (i + N k)] (q = sdim + 1; what: GDCA_MUT_DELTA | GDCA_MUT_POTENTIAL) of the K sequences packed by gdca_launch_energy_pack
// (Xg) from the element-wise lower triangle of A (ld; sign -1: A holds -mJ) and g = mJ Pi (gdca_launch_energy_g)
hipError_t gdca_launch_mutation_scan(hipStream_t s, const double *A, size_t ld, double sign, const double *g, const uint32_t *Xg, int N, int sdim,
                               int K, int what, double *D, int ncu);

// ---- k_epistasis.hip: the double-mutant scan -- best double substitution and epistasis strength of every site pair, listed double mutants ---
// (include/gdca.h, double-mutant scan).  Xg: the K sequences packed by gdca_launch_energy_pack; D: dE [K][N][q] of
// gdca_launch_mutation_scan (what = GDCA_MUT_DELTA); A, ld, sign as there.
#define GDCA_EPI_MAX_GROUPS (1LL << 24)  // workgroups one launch of the map kernel may have: ceil(K / 64) * T (T + 1) / 2, T = ceil(N / 4)
// Emin / code / epi [i + N (j + N k)], each may be nullptr.  generic: the instance with s at run time at s = 20 too.  An error: more
// workgroups than GDCA_EPI_MAX_GROUPS, or the dynamic LDS limit could not be raised; nothing was launched
hipError_t gdca_launch_double_mutant_scan(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, const double *D, int N,
                                          int sdim, int K, double *Emin, int32_t *code, double *epi, bool generic);
// out[r] = ddE of record r of muts (5 x L int32: k, i, b, j, c); a record out of range: GDCA_BAD_MUTANT in sc->bad_symbol, nothing indexed with it
void gdca_launch_double_mutants(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, const double *D,
                                const int32_t *muts, long long L, int N, int sdim, int K, double *out, gdca_dev_scalars *sc);

// ---- k_walk.hip: the greedy walk -- every sequence descends to a local energy minimum, one substitution a step ------------------------------
// (include/gdca.h, greedy walk).  Xg: the K sequences packed by gdca_launch_energy_pack; V: the site potentials [K][N][q] of
// gdca_launch_mutation_scan (what = GDCA_MUT_POTENTIAL); A, ld, sign as there.
#define GDCA_WALK_LDS_LIMIT (160 * 1024)  // LDS of a compute unit: what the table, the symbols and the reduction's slots may take together
size_t gdca_walk_lds_bytes(int N, int q, bool table_in_lds);
bool gdca_walk_table_fits(int N, int q);  // the instance with the table in LDS can run
// One workgroup a sequence.  table_in_lds: the table is copied to LDS, walked there and -- write_table -- written back to V at the end;
// else it is walked in place in V.  mask (N bytes), dE_sum, path, dE_path may be nullptr.  An error: the table does not fit, or the
// dynamic LDS limit could not be raised; nothing was launched
hipError_t gdca_launch_greedy_walk(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                                   const int8_t *mask, int flags, double min_gain, int max_steps, double *V, bool table_in_lds, bool write_table,
                                   int8_t *Xout, int32_t *steps, double *dE_sum, int32_t *path, double *dE_path);

// ---- k_sample.hip: Metropolis chains -- one workgroup a chain proposes single substitutions and accepts them at inverse temperature beta ---
// (include/gdca.h, Metropolis chains).  Xg, V, A, ld, sign as the walk's; the table is placed by the walk's rule (gdca_walk_table_fits:
// the LDS instance keeps the N s residue entries only, the gap's +0.0 is in the code, so what fits there fits here).
#define GDCA_SAMPLE_CHUNK_RULE 65536  // proposals a launch
// what a plain chain and a replica take alike (csrc/gdca_chain.h runs it)
struct gdca_chain_plan {
    const int8_t *mask;  // [N] or nullptr
    int flags;
    unsigned long long seed, stream0;
    int burn, stride, n_samples;
    double *thr;     // [chains][n_steps] or nullptr (a replica is a chain here)
    int32_t *moves;  // [chains][n_steps] or nullptr
    int n_steps() const { return burn + n_samples * stride; }
};
struct gdca_sample_plan {
    gdca_chain_plan chain;
    double beta;
    int8_t *Xs;         // [K][n_samples][N]
    double *dE_s;       // [K][n_samples] or nullptr
    int32_t *accepted;  // [K]: the count so far between two launches
};
// what both chain launchers check before they launch: the fit, the LDS limit, N, 0 <= t0 < t1 <= n_steps; *lds: the launch's dynamic LDS
hipError_t gdca_chain_launch_check(int N, int sdim, bool table_in_lds, const gdca_chain_plan &c, int t0, int t1, size_t *lds);
// what a chain keeps in HBM between two launches beside its table and `accepted`: the running sums (K doubles), then the symbols (K N bytes)
size_t gdca_sample_state_bytes(int N, int K);
// The proposals t0 .. t1 - 1 of every chain; t0 == 0 starts from Xg, a later launch from `state`.  table_in_lds: the table is copied
// to LDS and written back to V at the end of the launch, else it is updated in place.  An error: the table or the site list does not
// fit, or the dynamic LDS limit could not be raised; nothing was launched
hipError_t gdca_launch_sample(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                              const gdca_sample_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state);

// ---- k_temper.hip: replica exchange over the Metropolis chains -- R replicas a chain, one workgroup a replica, swap rounds between launches --
// (include/gdca.h, Replica-exchange chains).  G = K R replicas; Xg, V, A, ld, sign and the table's placement as k_sample's.
struct gdca_temper_plan {
    gdca_chain_plan chain;          // thr, moves: [K][R][n_steps]; n_rounds = n_steps / swap_every
    int R, swap_every;
    double betas[GDCA_TEMPER_MAX];  // HOST values, by slot; they travel as kernel arguments
    const int32_t *slot0;           // [K][R] or nullptr
    int8_t *Xs;                     // [K][n_samples][N]
    double *E_s;                    // [K][n_samples] or nullptr
    int32_t *accepted;              // [K][R], by slot
    int32_t *swaps;                 // [K][R - 1]
    int8_t *Xr_out;                 // [K][R][N]
    int32_t *slot_out;              // [K][R]
    double *swap_thr;               // [K][R - 1][n_rounds] or nullptr
    int32_t *slot_path;             // [K][R][n_rounds] or nullptr
};
// what the replicas keep in HBM beside their tables: the running sums, E0, the maps slot_of and holder, the symbols
size_t gdca_temper_state_bytes(int N, int G);
double *gdca_temper_E0(void *state, int G);  // where the stage writes the start energies (G doubles)
void gdca_launch_temper_replicate(hipStream_t s, const int8_t *X, int N, int K, int R, int8_t *Xr);
// the maps from slot0 (checked: GDCA_BAD_SLOTS in sc->bad_symbol, the identity in its place), accepted and swaps zeroed
void gdca_launch_temper_init(hipStream_t s, const gdca_temper_plan &plan, int K, void *state, gdca_dev_scalars *sc);
// The proposals t0 .. t1 - 1 of every replica, which may not cross a round (t0 / swap_every == (t1 - 1) / swap_every); errors as
// gdca_launch_sample's
hipError_t gdca_launch_temper_chain(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                                    const gdca_temper_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state);
// round e of every chain; js >= 0: the round is the point of sample js
void gdca_launch_temper_round(hipStream_t s, int N, int K, const gdca_temper_plan &plan, int e, int js, void *state);
void gdca_launch_temper_finish(hipStream_t s, int N, int K, const gdca_temper_plan &plan, void *state);

// ---- k_ais.hip: log partition function by annealed importance sampling -- one workgroup a chain along a ladder of inverse temperatures --
// (include/gdca.h, Log partition function).  Xg, V, A, ld, sign and the table's placement as k_sample's.
struct gdca_ais_plan {
    gdca_chain_plan chain;  // burn 0, stride = sweep, n_samples = L; thr, moves: [K][n_steps]
    int L, sweep;
    const double *betas;    // [L + 1], DEVICE
    double *out4, *logw;    // [4], [K]
    double *E_end;          // [K] or nullptr
    int8_t *X0, *Xout;      // [K][N] or nullptr each
    int32_t *accepted;      // [K] or nullptr
};
// what the chains keep in HBM beside their tables: the running sums, the log-weights, E0, the counts, the length of the site list, the symbols
size_t gdca_ais_state_bytes(int N, int K);
double *gdca_ais_E0(void *state, int K);  // where the stage writes the start energies (K doubles)
// the uniform starts of the K chains from the template x (nullptr: every site is free) into Xst (N x K) and, where asked, plan.X0
void gdca_launch_ais_start(hipStream_t s, const int8_t *x, int N, int q, int K, const gdca_ais_plan &plan, int8_t *Xst, void *state);
// The proposals t0 .. t1 - 1 of every chain, each at the beta of its stage; the last launch writes the outputs; errors as gdca_launch_sample's
hipError_t gdca_launch_ais(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                           const gdca_ais_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state);
// plan.out4 from plan.logw; T: the target symbols of a site
void gdca_launch_ais_reduce(hipStream_t s, int K, int T, const gdca_ais_plan &plan, void *state);

// ---- k_bm.hip: Boltzmann-machine refinement -- the warm start, the parameter update and the fit read-out of the Potts model (W, 0) ------
// (include/gdca.h, Boltzmann-machine refinement).  Every matrix is n x n column-major with ld = n, n = N sdim.
// W from the lower triangle of mJ and g = mJ Pi (gdca_launch_energy_g); W may not alias mJ
void gdca_launch_bm_from_gaussian(hipStream_t s, const double *mJ, const double *g, int N, int sdim, double *W);
// one pass over W in place: W = W + eta (m (Pij_m - Pij_d) - [m == 1] lambda W), entry by entry
void gdca_launch_bm_update(hipStream_t s, double *W, const double *Pij_d, const double *Pij_m, int N, int sdim, double eta, double lambda);
// out[0 .. 2] (out[3] = +0.0 where zero3) through `part`, gdca_bm_readout_bytes(n) bytes of workspace
size_t gdca_bm_readout_bytes(int n);
void gdca_launch_bm_readout(hipStream_t s, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int N, int sdim,
                            double *part, double *out, bool zero3);
// *out = (sum of accepted[0 .. K - 1]) / (K n_steps)
void gdca_launch_bm_accept(hipStream_t s, const int32_t *accepted, int K, long long n_steps, double *out);
// X (N x K) <- the last of the n_samples samples of every chain in Xs (k_sample's layout)
void gdca_launch_bm_last_sample(hipStream_t s, const int8_t *Xs, int N, int K, int n_samples, int8_t *X);
void gdca_launch_bm_fill(hipStream_t s, double *v, size_t count, double value);

// ---- k_plm.hip: pseudo-likelihood fit of the Potts model (W, 0) -- the conditionals of the mutation stage's potentials, their tally against
// the alignment, the finish (include/gdca.h, Pseudo-likelihood) -----------------------------------------------------------------------------
#define GDCA_PLM_CHUNK_RULE 512  // sequences a block of the tally
// D [K][N][q] from V to p in place, l_ki into L [K][N], nll_k [K]; Xg the K sequences' packed symbols
void gdca_launch_plm_softmax(hipStream_t s, double *D, const uint32_t *Xg, int N, int K, int q, double *L, double *nll_k);
// Q (n x n) and S (n), +0.0 before the first slab, take a slab of K sequences in, blocks of `chunk`; an error: nothing launched
hipError_t gdca_launch_plm_tally(hipStream_t s, const double *p, const uint32_t *Xg, const double *w, int N, int sdim, int K, int chunk,
                                 double *Q, double *S);
void gdca_launch_plm_finish(hipStream_t s, const double *Q, const double *S, int N, int sdim, double Meff, double *Pi, double *Pij);
// *out = (sum_k w_k nll_k) / Meff by one workgroup's fixed tree
void gdca_launch_plm_nll(hipStream_t s, const double *w, const double *nll_k, int M, double Meff, double *out);
// a weight outside [0, 1]: GDCA_BAD_WEIGHT in sc->bad_symbol
void gdca_launch_plm_check_weights(hipStream_t s, const double *w, int M, gdca_dev_scalars *sc);
