// C-ABI of libgdca.so (see include/gdca.h): context, workspace, the fused device pipeline and
// the operator-level entry points.  Host-side orchestration only; all arithmetic is in the
// k_*.hip kernels.  No CPU fallback exists: every entry point needs a HIP device.
#include <algorithm>
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "gdca_hamming_form.h"
#include "gdca_internal.h"
#include "gdca_sweep_schedule.h"
#include "gdca_launch.h"

struct gdca_buf {
    void *p;
    size_t cap;
};

// The device buffers behind the arrays of a host-pointer call (host_stage, below): the context's, grow-only, one per array in the order
// a call asks for them.  Only host_stage can name them; gdca_ctx_destroy frees them through release().
class stage_pool {
    friend class host_stage;
    static const int MAX_ARRAYS = 16;
    gdca_buf buf[MAX_ARRAYS];

public:
    void release()
    {
        for (gdca_buf &b : buf)
            if (b.p) (void)hipFree(b.p);
    }
};

// Shared by the contexts of one pipeline (gdca_ctx_create_peer): orders their SPD-inverse stages one after
// the other on the device, so that only the non-MFMA stages of the next family overlap the inverse of the
// current one (two interleaved inverses would just halve each other's MFMA rate).
struct gdca_gate {
    hipEvent_t ev[4];
    int next, last, armed, refs;
    // the pipeline's own stream: every phase batch issued as batched grids by a member of the pipeline goes here, so that the batches
    // of two alternating context sets are ONE in-order sequence -- two streams that share a hardware queue take turns with hundreds
    // of microseconds between them (400 us measured between one set's score stage and the other's front end at config B), and on
    // different hardware queues the next batch's small kernels become resident beside the running persistent sweep
    hipStream_t batch_stream;
};

// What the score stage of a run computes, handed to score_stage by whoever calls it: the contact score (FN or DI, with or without
// APC), or -- the fused energy entries -- the model scored on sequences X, on the pairings across a split, or scanned for every single
// substitution of sequences X; LOGLIK is the energy target whose E the collect turns into log-likelihoods once the run's log det is on
// the host (loglik_epilogue).  The enqueued run keeps
// its own (gdca_pending::target): a second attempt, refinement or fallback at collect time scores the same thing again.
// The species of a species-sorted pair problem as the blocked pair stage and the assignment take them (species_blocks makes it): the
// species table and the gather's work list on the device (ctx->PBtab, ctx->PBitems), and what the host keeps of them.
struct pair_blocks {
    const long long *eoff;         // device [S + 1]: where block s starts in the packed matrix
    const int32_t *offA, *offB;    // device [S + 1] each
    const int32_t *items;          // device: the work list (gdca_pair_block_items), cut for chunks of Ac sequences a
    const long long *first;        // HOST: the first item of every chunk of T, and the count behind the last (valid during the call)
    int S, Ac, kmax;               // kmax: the largest kA_s or kB_s
    long long total;               // doubles of the packed matrix
};

// What a greedy walk takes beside its sequences and returns (include/gdca.h, greedy walk): device pointers, each but Xout and steps
// may be nullptr
struct walk_request {
    const int8_t *mask;
    int flags, max_steps;
    double min_gain;
    int8_t *Xout;
    int32_t *steps;
    double *dE_sum;
    int32_t *path;
    double *dE_path;
    double *V;
};

// What the Metropolis chains take beside their start sequences and return (include/gdca.h, Metropolis chains): the kernel's plan and
// the final tables; device pointers, dE_s, thr, moves and V may be nullptr
struct sample_request {
    gdca_sample_plan plan;
    double *V;
};

// What the replica-exchange chains take beside their start sequences and return (include/gdca.h, Replica-exchange chains): the
// kernels' plan, with the ladder by value (a collect that runs the stage again needs no array of the caller's).  fused: the start
// sequences are N x K and every replica of a chain starts at its chain's; else they are N x R x K
struct temper_request {
    gdca_temper_plan plan;
    bool fused;
};

struct score_target {
    enum { CONTACT, ENERGY, PAIR, PARTNER, MUTATION, LOGLIK, DOUBLE_SCAN, DOUBLE_LIST, WALK, SAMPLE, TEMPER } kind;
    double *out;                       // S (N x N), E (K), E (KA x KB), E (packed blocks), D (q x N x K), Emin (N x N x K, may be null) or ddE (L)
    int score, apc;                    // contact
    const int8_t *X;                   // energy (k_energy.hip) and mutation scan (k_mutation.hip, with `what`): N x K
    int K;
    const int8_t *XA, *XB;             // pair (k_pair_energy.hip): as pair_stage takes them
    size_t strideA, strideB;
    int KA, KB, split, what;
    pair_blocks blocks;                // partner: the blocked pair stage, then the assignment (k_assign.hip) into match / gap
    int32_t *match;
    double *gap;
    bool packed;                       // partner: XA / XB lie packed and padded in the context already (pair_pack; the rounds of gdca_run_partner_ipa)
    size_t strideX;                    // energy: bytes from one sequence of X to the next (0: N -- whole sequences)
    int32_t *dcode;                    // double-mutant scan (k_epistasis.hip): the maps beside Emin (`out`), each may be null
    double *depi;
    const int32_t *muts;               // listed double mutants: 5 x L records
    int L;
    walk_request walk;                 // greedy walk (k_walk.hip) of the sequences X: the rule's parameters and the outputs
    sample_request sample;             // Metropolis chains (k_sample.hip) from the sequences X: the rule's parameters and the outputs
    temper_request temper;             // replica-exchange chains (k_temper.hip) from the sequences X
    // pair / partner of a log-odds run (run_logodds): the pair stage waits for the collect, which knows the joint log det (logodds_epilogue);
    // lo.EmA / lo.EmB: the marginal fits' energies, ldA / ldB their log dets, lo.I what the collect makes of the three
    bool logodds;
    gdca_logodds_terms lo;
    double ldA, ldB;
};

static score_target contact_target(int score, int apc, double *S_dev)
{
    score_target t{};
    t.kind = score_target::CONTACT;
    t.out = S_dev;
    t.score = score;
    t.apc = apc;
    return t;
}

// The read-outs of the fused entries: X == NULL (XA / XB likewise) means the alignment's own M sequences -- for a pair target their
// halves as they lie in Z (N x M), N bytes apart.
static score_target energy_target(const int8_t *Z, int M, const int8_t *X, int K, double *E_dev)
{
    score_target t{};
    t.kind = score_target::ENERGY;
    t.out = E_dev;
    t.X = X ? X : Z;
    t.K = X ? K : M;
    return t;
}

// (the energies of the same sequences; what the collect makes of them: gdca_run_collect)
static score_target loglik_target(const int8_t *Z, int M, const int8_t *X, int K, double *L_dev)
{
    score_target t = energy_target(Z, M, X, K, L_dev);
    t.kind = score_target::LOGLIK;
    return t;
}

static score_target pair_target(const int8_t *Z, int N, int M, int split, const int8_t *XA, int KA, const int8_t *XB, int KB, int what,
                                double *E_dev)
{
    score_target t{};
    t.kind = score_target::PAIR;
    t.out = E_dev;
    t.split = split;
    t.what = what;
    t.XA = XA ? XA : Z;
    t.strideA = XA ? (size_t)split : (size_t)N;
    t.KA = XA ? KA : M;
    t.XB = XB ? XB : Z + split;
    t.strideB = XB ? (size_t)(N - split) : (size_t)N;
    t.KB = XB ? KB : M;
    return t;
}

// (the pair target's sequences; the species come sorted as blk describes them)
static score_target partner_target(const score_target &pair, const pair_blocks &blk, int32_t *match_dev, double *gap_dev)
{
    score_target t = pair;
    t.kind = score_target::PARTNER;
    t.blocks = blk;
    t.match = match_dev;
    t.gap = gap_dev;
    return t;
}

static score_target mutation_target(const int8_t *Z, int M, const int8_t *X, int K, int what, double *D_dev)
{
    score_target t = energy_target(Z, M, X, K, D_dev);
    t.kind = score_target::MUTATION;
    t.what = what;
    return t;
}

// (X is never the alignment itself here: N^2 M outputs are not on offer)
static score_target double_scan_target(const int8_t *X, int K, double *Emin_dev, int32_t *code_dev, double *epi_dev)
{
    score_target t{};
    t.kind = score_target::DOUBLE_SCAN;
    t.out = Emin_dev;
    t.dcode = code_dev;
    t.depi = epi_dev;
    t.X = X;
    t.K = K;
    return t;
}

static score_target double_list_target(const int8_t *X, int K, const int32_t *muts_dev, int L, double *out_dev)
{
    score_target t{};
    t.kind = score_target::DOUBLE_LIST;
    t.out = out_dev;
    t.muts = muts_dev;
    t.L = L;
    t.X = X;
    t.K = K;
    return t;
}

// (X == NULL: the alignment's own M sequences)
static score_target walk_target(const int8_t *Z, int M, const int8_t *X, int K, const walk_request &w)
{
    score_target t = energy_target(Z, M, X, K, nullptr);
    t.kind = score_target::WALK;
    t.walk = w;
    return t;
}

// (X == NULL: one chain from each of the alignment's own M sequences)
static score_target sample_target(const int8_t *Z, int M, const int8_t *X, int K, const sample_request &r)
{
    score_target t = energy_target(Z, M, X, K, nullptr);
    t.kind = score_target::SAMPLE;
    t.sample = r;
    return t;
}

// (X == NULL: one chain from each of the alignment's own M sequences)
static score_target temper_target(const int8_t *Z, int M, const int8_t *X, int K, const temper_request &r)
{
    score_target t = energy_target(Z, M, X, K, nullptr);
    t.kind = score_target::TEMPER;
    t.temper = r;
    return t;
}

// The enqueued, not yet collected run (gdca_run_dev_async / gdca_run_collect): all a collect needs to know, grouped by who writes it.
// The operator-level inverse (gdca_spd_inverse_dev, gdca_spd_inverse_batch_dev) borrows n, n_pad, timed (false: begin()) and the
// progress record `at` -- attempt and refined --, so that it can go through run_inverses and inverse_ladder.
struct gdca_pending {
    // ---- the front end (pending_front) ----
    int N, M, q, n, n_pad;
    const int8_t *Z;           // what a refinement at collect time needs to build C again
    const double *pij;         // ... or, a pseudocount group of gdca_run_multi, the stored Pij_true C is built again from (nullptr: the tallies)
    int N_all, site0;          // a marginal fit of a log-odds run: N is a range of the sites of an alignment of N_all, from site0 on; pij the joint Pij_true (N_all 0: no range)
    gdca_params p;
    // the run's timeline (open_timeline, mark, elapsed): whether it is timed at all, its clock -- device time stamps for a member of a
    // batch issued as batched grids, HIP events otherwise --, and which boundaries have been marked so far, by which of the two clocks
    bool timed, stamped;
    unsigned ev_marks, stamp_marks;
    int front_batch;           // members that shared this run's batched front-end grids (1: grids of its own); their stage times are the grids' divided by it
    int score_batch;           // ... and its score grids (run_phased sets both; 1 again once the stage has run alone at collect time)
    // ---- the inverse (run_inverse, run_inverse_merged) ----
    int n_upd;
    int batch;                 // families that shared this run's SPD-inverse launch (1: a launch of its own)
    double upd_flops;
    // ---- the score stage (run_score) ----
    score_target target;
    bool sc_published;         // the run ends with k_publish_scalars: its collect reads sc_host after a stream synchronisation
    // ---- progress at collect time (zero when a run begins) ----
    struct progress {
        int attempt;           // attempts the run's inverse has had so far (0: the first is enqueued); its watchdog may end a launch (k_inverse.hip, spin_until)
        bool rescored;         // ... and it was run again at collect time: the scores (and a ranking) are those of the last attempt
        int refined;           // what the ladder did to the inverse (gdca_stats.refined; the codes: gdca_refined_after_step)
    } at;
    // ---- a ranked run (gdca_run_ranked_async): where its ranking will be, and whether enqueueing it worked ----
    struct {
        bool pending;
        long long len;
        int sep;
        gdca_status status;
        int32_t *i, *j;
        double *s;
    } rank;
};

struct gdca_ctx {
    int device;
    gdca_gate *gate;
    hipStream_t stream;
    bool own_stream;
    bool timing;
    gdca_tuning tune;          // this context's switches (gdca_ctx_set_option; GDCA_* environment at creation)
    char err[512];
    // named device buffers (grow-only)
    gdca_buf Zt, Zp, hist, Zb, hcnt, nk, W, Wfix, Pifix, Pipc, A, G, H, P, Sg, Dblk, Ld, Tws, colsum, sc;
    gdca_buf normws, C2, B0, Rt;  // ||X||_1 workspace; Newton-Schulz refinement (allocated when a run first needs it): C again, X0 in full, I - X0 C
    gdca_buf Wd;                  // Cholesky fallback: the inverses of the diagonal tiles of the factor
    gdca_buf hcand;               // reweighting, bound forms: the list of candidate pairs
    gdca_buf himg;                // reweighting, consensus form: the image of the consensus plane as E2M1 nibbles, and sigma
    gdca_buf rankws;              // device ranking: keys, values, histograms, the three output arrays
    gdca_buf keep;                // pair tally, TALLY_SKIP: the sequences each column's tally visits, their counts and sigma (k_pi_keep)
    gdca_buf Pij;                 // gdca_run_multi: Pij_true of the alignment (n x n, ld = n), the covariance of every pseudocount is built from it
    gdca_buf sc_front;            // gdca_run_multi: the scalars as the front end left them (every pseudocount group starts from them)
    gdca_buf Xg, Epart, gpart, gvec;  // energies (k_energy.hip): the packed sequences, the per-site-block partial energies, the partials of g = mJ Pi, g and c0
    // pair energies (k_pair_energy.hip): the packed symbols of the A and the B halves, the gap-padded halves and their marginal energies,
    // the folded rows T of one chunk of A sequences
    gdca_buf PXa, PXb, PXpad, PEab, PT;
    // partner matching: the species table (eoff, offA, offB), the blocked gather's work list, and the packed matrix of a fused run
    // whose caller does not want it
    gdca_buf PBtab, PBitems, PBE;
    // pair log-odds: the marginal models' energies of the A and of the B sequences, and -L in packed blocks for the assignment
    gdca_buf LOa, LOb, PBN;
    // iterative partner matching (k_ipa.hip): the selection's workspace (keys, values, histograms, flags), the counts a round hands to
    // the host, the growing training alignment, the selection (and a seed's partners behind it), a round's match / gap, the match of
    // the round before, and the species of every sequence a
    gdca_buf IPAws, IPAcnt, IPAZ, IPAsel, IPAm, IPAg, IPAprev, IPAsp;
    gdca_buf DMd;             // double-mutant scan (k_epistasis.hip): dE of every single substitution of its sequences, q N K doubles
    gdca_buf SMst;            // Metropolis chains (k_sample.hip): what a chain keeps between two launches, gdca_sample_state_bytes
    // Boltzmann-machine refinement (k_bm.hip): the loop's workspace (bm_plan: the model's tallies, the zero Pi, the unit weights, the
    // counts, the samples), and the read-out's column partials
    gdca_buf TMst, TMx;       // replica-exchange chains (k_temper.hip): gdca_temper_state_bytes, and the fused form's N x R x K starts
    gdca_buf BMws, BMred;
    // log partition function (k_ais.hip): gdca_ais_state_bytes, the N x K starts, the ladder's L + 1 betas
    gdca_buf AISst, AISx, AISb;
    // pseudo-likelihood fit (k_plm.hip): the slab's table of potentials / conditionals, and plm_plan's arrays
    gdca_buf PLMv, PLMws;
    int ncu;                  // compute units of the device
    double *piv;              // the pivots of the context's last inverse, n_pad doubles inside Sg (inverse_job)
    // log det of the matrix of the last SPD inverse this context completed (gdca_last_logdet): kept on the host, so that entry points
    // without an inverse of their own (their begin() clears the device scalars) leave it alone.  count: 0 = none, K after gdca_run_multi;
    // chol: the Cholesky fallback factored that matrix (its diagonal is what the pivot vector holds)
    struct {
        int count;
        bool chol;
        double val[GDCA_MULTI_MAX];
        int src[GDCA_MULTI_MAX];
    } ld;
    int *item0_host;           // pinned staging of the sweep's item table
    int item0_cap;
    stage_pool staging;        // the arrays of a host-pointer call (host_stage)
    gdca_dev_scalars *sc_host;  // pinned
    gdca_dev_scalars *sc_host_dev;  // ... as the device addresses it (k_publish_scalars)
    hipEvent_t ev[T_COUNT];    // the stage boundaries of a timed run (made when the first one opens its timeline)
    hipEvent_t ev_batch, ev_upload;
    bool pending;              // a run is enqueued and not yet collected ...
    gdca_pending pend;         // ... this one
};

// ---- batched grids: the recorder of gdca_launch.h, and the two stream operations of this file in recordable form ------------------
gdca_recorder *&gdca_recorder::active()
{
    static thread_local gdca_recorder *r = nullptr;
    return r;
}

void gdca_recorder::begin(hipStream_t s, int members)
{
    stream = s;
    lists.assign((size_t)members, {});
    cur = -1;
    active() = this;
}

void gdca_recorder::add(const gdca_op &op)
{
    lists[(size_t)cur].push_back(op);
    ++ops;
}

hipError_t gdca_recorder::flush()
{
    const int K = (int)lists.size();
    std::vector<size_t> at((size_t)K, 0);
    hipError_t err = hipSuccess;
    const int keep = cur;
    cur = -1;  // (the launchers below go out at once)
    for (;;) {
        int k0 = -1;
        for (int k = 0; k < K; ++k)
            if (at[k] < lists[k].size() && (k0 < 0 || at[k] < at[k0])) k0 = k;
        if (k0 < 0) break;
        // the kind at the head of the list of the member that has got least far, and every member whose head is of that kind
        const gdca_op &h = lists[k0][at[k0]];
        const gdca_op *grp[GDCA_MAXB];
        int n = 0;
        for (int k = 0; k < K && n < GDCA_MAXB; ++k) {
            if (at[k] >= lists[k].size()) continue;
            const gdca_op &o = lists[k][at[k]];
            if (o.launch != h.launch || o.block.x != h.block.x || o.block.y != h.block.y || o.block.z != h.block.z) continue;
            grp[n++] = &o;
            ++at[k];
        }
        h.launch(stream, grp, n);
        ++launches;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess && err == hipSuccess) err = e;
    }
    for (auto &l : lists) l.clear();
    cur = keep;
    return err;
}

hipError_t gdca_recorder::end()
{
    const hipError_t e = flush();
    active() = nullptr;
    cur = -1;
    return e;
}

struct k_fill32_args {
    unsigned *p;
    unsigned v;
    size_t words;
};
template <int CAP>
__global__ __launch_bounds__(256) void k_fill32(const BatchArgs<k_fill32_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    unsigned *__restrict__ p = a_.p;
    const unsigned v = a_.v;
    const size_t words = a_.words;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = v;
}

// hipMemsetAsync for buffers of whole 32-bit words; while the calling thread records a batch, a kernel of the batch
void gdca_fill_async(hipStream_t s, void *p, int byte_value, size_t bytes)
{
    gdca_recorder *r = gdca_recorder::active();
    if (!r || r->cur < 0 || s != r->stream || (bytes & 3) || ((uintptr_t)p & 3)) {
        GDCA_FLUSH_RECORDED();
        (void)hipMemsetAsync(p, byte_value, bytes, s);
        return;
    }
    const size_t words = bytes / 4;
    const unsigned v = (unsigned)(byte_value & 0xff) * 0x01010101u;
    const unsigned grid = (unsigned)std::min<size_t>((words + 255) / 256, 1024);
    if (grid) gdca_launch<k_fill32_args, k_fill32<1>, k_fill32<GDCA_MAXB>>(dim3(grid), dim3(256), 0, s, k_fill32_args{(unsigned *)p, v, words});
}

struct k_stamp_args {
    gdca_dev_scalars *sc;
    int slot, slot2;  // gdca_boundary (slot2: T_NONE for one slot)
};
template <int CAP>
__global__ __launch_bounds__(64) void k_stamp(const BatchArgs<k_stamp_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    if (threadIdx.x == 0) {
        const unsigned long long t = wall_clock64();
        a_.sc->stamp[a_.slot] = t;
        if (a_.slot2 >= 0) a_.sc->stamp[a_.slot2] = t;
    }
}

void gdca_launch_stamp(hipStream_t s, gdca_dev_scalars *sc, int slot, int slot2)
{
    gdca_launch<k_stamp_args, k_stamp<1>, k_stamp<GDCA_MAXB>>(dim3(1), dim3(64), 0, s, k_stamp_args{sc, slot, slot2});
}

// ---- tuning switches: environment at context creation, gdca_ctx_set_option afterwards -----------------------------------------
static bool parse_long(const char *v, long *out)
{
    if (!v || !*v) return false;
    char *end = nullptr;
    const long x = strtol(v, &end, 10);
    if (end == v || *end) return false;
    *out = x;
    return true;
}

bool gdca_tuning_set(gdca_tuning *t, const char *key, const char *value)
{
    if (!t || !key || !value) return false;
    char k[64];
    size_t n = 0;
    if (!strncasecmp(key, "GDCA_", 5)) key += 5;
    for (; key[n] && n + 1 < sizeof(k); ++n) k[n] = (char)toupper((unsigned char)key[n]);
    k[n] = 0;
    if (!strcmp(k, "SWEEP_TRACE")) {
        if (strlen(value) >= sizeof(t->sweep_trace)) return false;
        strcpy(t->sweep_trace, value);
        return true;
    }
    if (!strcmp(k, "HAMMING_MODE")) {
        const char c = (char)tolower((unsigned char)value[0]);
        t->hamming_mode = c == 'f' ? 0 : (c == 'b' ? 1 : (c == 'm' ? 2 : -1));
        return c == 'f' || c == 'b' || c == 'm' || c == 'a' || c == 0;  // full | bound | mfma | auto
    }
    if (!strcmp(k, "WALK_TABLE")) {  // auto | lds | hbm
        const int v = !strcasecmp(value, "auto") ? 0 : (!strcasecmp(value, "lds") ? 1 : (!strcasecmp(value, "hbm") ? 2 : -1));
        if (v < 0) return false;
        t->walk_table = v;
        return true;
    }
    if (!strcmp(k, "FORCE_FALLBACK")) {  // any value but "" and "0" switches it on (as DCAUTILS_FORCE_FALLBACK in the reference's tests)
        t->force_fallback = (*value && strcmp(value, "0") != 0) ? 1 : 0;
        return true;
    }
    long x = 0;
    if (strcmp(k, "REFINE") && strcmp(k, "REFINE_COND") && !parse_long(value, &x)) return false;
    struct { const char *name; int *field; long lo, hi; } ints[] = {
        {"GROUP", &t->group, -1, 4},        {"RAMP", &t->ramp, 0, 1},          {"RAGGED", &t->ragged, 0, 1},
        {"REM_TAIL", &t->rem_tail, -1, 1 << 20}, {"PANEL_HALVES", &t->panel_halves, -1, 1}, {"SLAB", &t->slab, 0, 1},
        {"RING", &t->ring, 2, 8},           {"MCUS", &t->mcus, -1, 32},        {"MCU_SOLO", &t->mcu_solo, -1, 1},       {"SWEEP_DEBUG", &t->sweep_debug, 0, 63}, {"SWEEP_RETRIES", &t->sweep_retries, 0, 5},
        {"HAM_CUT", &t->ham_cut, 0, 1 << 20}, {"TALLY_TJ", &t->tally_tj, 0, 32},  {"TALLY_SKIP", &t->tally_skip, 0, 1}, {"MERGE", &t->merge, 1, 8},        {"MERGE_BLOCKS", &t->merge_blocks, 1, 64},
        {"MERGE_MCUS", &t->merge_mcus, -1, 16},  {"MERGE_GROUP", &t->merge_group, -1, 4}, {"MERGE_TILES", &t->merge_tiles, 1, 1 << 20},
        {"CHOLESKY", &t->cholesky, 0, 2},  {"PHASED_FRONTS", &t->phased_fronts, 0, 1}, {"PHASED_GRIDS", &t->phased_grids, -1, 8}, {"PHASED_STREAMS", &t->phased_streams, 1, 64},
        {"ENERGY_CHUNK", &t->energy_chunk, 0, 1 << 30}, {"PAIR_CHUNK", &t->pair_chunk, 0, 1 << 30},
        {"EPI_GENERIC", &t->epi_generic, 0, 1}, {"SAMPLE_CHUNK", &t->sample_chunk, 0, INT32_MAX},
        {"PLM_CHUNK", &t->plm_chunk, 0, 1 << 20}, {"PLM_SLAB", &t->plm_slab, 0, INT32_MAX},
    };
    for (auto &e : ints)
        if (!strcmp(k, e.name)) {
            if (x < e.lo || x > e.hi) return false;
            *e.field = (int)x;
            return true;
        }
    if (!strcmp(k, "REFINE")) {
        const char c = (char)tolower((unsigned char)value[0]);
        if (c == 'a' || !strcmp(value, "-1")) t->refine = -1;
        else if (!strcmp(value, "0") || !strcasecmp(value, "off") || c == 'n') t->refine = 0;
        else if (!strcmp(value, "1") || !strcasecmp(value, "on") || c == 'y') t->refine = 1;
        else return false;
        return true;
    }
    if (!strcmp(k, "REFINE_COND")) {
        char *end = nullptr;
        const double x = strtod(value, &end);
        if (end == value || *end || !(x > 0.0)) return false;
        t->refine_cond = x;
        return true;
    }
    if (!strcmp(k, "SWEEP_TIMEOUT_MS")) {
        if (x < 0) return false;
        t->sweep_timeout_ms = x;
        return true;
    }
    return false;
}

void gdca_tuning_from_env(gdca_tuning *t)
{
    memset(t, 0, sizeof(*t));
    t->group = -1;
    t->ramp = 1;
    t->ragged = 1;
    t->rem_tail = -1;
    t->panel_halves = -1;
    t->slab = 1;
    t->ring = 8;
    t->mcus = -1;
    t->mcu_solo = -1;
    t->sweep_retries = 2;
    t->tally_skip = 1;
    t->hamming_mode = -1;
    t->merge = 8;
    t->merge_blocks = 57;
    t->merge_mcus = -1;
    t->merge_group = -1;
    t->merge_tiles = 2300;
    t->phased_fronts = 1;
    t->phased_grids = -1;
    t->phased_streams = 4;
    t->refine = -1;
    t->refine_cond = 1e6;
    t->cholesky = 1;
    static const char *const names[] = {"GDCA_GROUP", "GDCA_RAMP", "GDCA_RAGGED", "GDCA_REM_TAIL", "GDCA_PANEL_HALVES", "GDCA_SLAB",
                                        "GDCA_RING", "GDCA_MCUS", "GDCA_SWEEP_DEBUG", "GDCA_SWEEP_TIMEOUT_MS", "GDCA_SWEEP_RETRIES", "GDCA_TALLY_TJ", "GDCA_TALLY_SKIP",
                                        "GDCA_HAMMING_MODE", "GDCA_HAM_CUT", "GDCA_FORCE_FALLBACK", "GDCA_MERGE", "GDCA_MERGE_BLOCKS",
                                        "GDCA_MERGE_MCUS", "GDCA_MERGE_GROUP", "GDCA_MERGE_TILES", "GDCA_REFINE", "GDCA_REFINE_COND", "GDCA_CHOLESKY", "GDCA_SWEEP_TRACE", "GDCA_PHASED_FRONTS", "GDCA_PHASED_GRIDS", "GDCA_PHASED_STREAMS", "GDCA_MCU_SOLO", "GDCA_ENERGY_CHUNK", "GDCA_PAIR_CHUNK", "GDCA_EPI_GENERIC", "GDCA_WALK_TABLE", "GDCA_SAMPLE_CHUNK", "GDCA_PLM_CHUNK", "GDCA_PLM_SLAB"};
    for (const char *nm : names)
        if (const char *v = getenv(nm)) (void)gdca_tuning_set(t, nm, v);  // an unusable value leaves the default
}

static gdca_status fail(gdca_ctx *ctx, gdca_status st, const char *fmt, const char *a, const char *b)
{
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), fmt, a, b);
    return st;
}

// ... with a fixed text
static gdca_status fail(gdca_ctx *ctx, gdca_status st, const char *text)
{
    return fail(ctx, st, "%s%s", text, "");
}

// how a call that has the device scalars in sc_host ends: the verdict on them (gdca_inverse_outcome.h) as status and last error
static gdca_status conclude(gdca_ctx *ctx, gdca_call_kind kind)
{
    const gdca_dev_scalars &h = *ctx->sc_host;
    const gdca_verdict v = gdca_verdict_of(kind, h.bad_symbol, h.info, h.di_noconv);
    return v.status == GDCA_OK ? GDCA_OK : fail(ctx, v.status, v.text);
}

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail(ctx, GDCA_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define CHK(expr)                         \
    do {                                  \
        gdca_status s_ = (expr);          \
        if (s_ != GDCA_OK) return s_;     \
    } while (0)

static gdca_status ensure(gdca_ctx *ctx, gdca_buf &b, size_t bytes)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return GDCA_OK;
    if (b.p) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(ctx, GDCA_ENOMEM, "hipMalloc failed: %s%s", hipGetErrorString(e), "");
    }
    b.cap = want;
    return GDCA_OK;
}

static gdca_status check_launch(gdca_ctx *ctx, const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, GDCA_EHIP, "launch %s: %s", what, hipGetErrorString(e));
    return GDCA_OK;
}

extern "C" {

int32_t gdca_version(void)
{
    return GDCA_VERSION_MAJOR * 1000 + GDCA_VERSION_MINOR;
}

int32_t gdca_stats_bytes(void)
{
    return (int32_t)sizeof(gdca_stats);
}

int32_t gdca_params_bytes(void)
{
    return (int32_t)sizeof(gdca_params);
}

int32_t gdca_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

gdca_status gdca_ctx_create_on_stream(int32_t device_id, void *hip_stream, gdca_ctx **out)
{
    if (!out) return GDCA_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GDCA_EHIP;
    if (device_id < 0 || device_id >= ndev) return GDCA_EINVAL;
    gdca_ctx *ctx = (gdca_ctx *)calloc(1, sizeof(gdca_ctx));
    if (!ctx) return GDCA_ENOMEM;
    ctx->device = device_id;
    ctx->timing = true;
    gdca_tuning_from_env(&ctx->tune);
    if (hipSetDevice(device_id) != hipSuccess) {
        free(ctx);
        return GDCA_EHIP;
    }
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    {
        hipDeviceProp_t prop0;
        ctx->ncu = hipGetDeviceProperties(&prop0, device_id) == hipSuccess ? prop0.multiProcessorCount : 256;
    }
    // from here on every failure goes through gdca_ctx_destroy, which frees whatever has been created so far
    if (hipEventCreateWithFlags(&ctx->ev_batch, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_upload, hipEventDisableTiming) != hipSuccess) {
        gdca_ctx_destroy(ctx);
        return GDCA_EHIP;
    }
    if (hipHostMalloc((void **)&ctx->sc_host, sizeof(gdca_dev_scalars), hipHostMallocDefault) != hipSuccess) {
        ctx->sc_host = nullptr;
        gdca_ctx_destroy(ctx);
        return GDCA_ENOMEM;
    }
    if (hipHostGetDevicePointer((void **)&ctx->sc_host_dev, ctx->sc_host, 0) != hipSuccess) ctx->sc_host_dev = nullptr;  // (then collect copies)
    *out = ctx;
    return GDCA_OK;
}

// A stream's hardware queue comes into being with the stream's FIRST command, not with the stream -- and the driver maps a new queue
// by taking every queue of the device off the hardware and putting them back: the waves of all running kernels are saved and restored
// (a standstill of ~1.7 ms, measured from inside the sweep kernel; the waves come back on other compute units).  Restored beside the
// kernels of other streams, a persistent sweep need not get all its workgroups back at once -- and those it did get back wait for
// the items the others hold, keeping the compute units those would need: the launch stands still until its watchdog ends it.
// Round 6's batch driver ran into exactly that, in 1 to 8 of 100 runs: the contexts of its phase batches were made when the first
// small family showed up, their streams started beside a slot's running sweep (tools/rounds/r06/gpu_r6q.sh, gpu_r6s.sh; made before
// any work: 0 of 200).  So the queue is made HERE, with the context -- one small fill and a synchronisation; the context's scalars
// are allocated on the way -- and callers make their contexts before they enqueue work (include/gdca.h).  What a caller cannot
// rule out (another process starting on the same GPU) is what the sweep's watchdog and gdca_run_collect's second attempt are for.
static gdca_status warm_stream(gdca_ctx *ctx, hipStream_t s)
{
    CHK(ensure(ctx, ctx->sc, sizeof(gdca_dev_scalars)));
    gdca_fill_async(s, ctx->sc.p, 0, sizeof(gdca_dev_scalars));
    if (hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GDCA_EHIP, "the context's stream could not be started");
    }
    return GDCA_OK;
}

gdca_status gdca_ctx_create(int32_t device_id, gdca_ctx **out)
{
    gdca_status st = gdca_ctx_create_on_stream(device_id, nullptr, out);
    if (st != GDCA_OK) return st;
    gdca_ctx *ctx = *out;
    // the context's own stream: non-blocking, at the highest priority the device offers (a family's kernels should not queue
    // behind whatever else the process runs on the device)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        gdca_ctx_destroy(ctx);
        *out = nullptr;
        return GDCA_EHIP;
    }
    ctx->own_stream = true;
    st = warm_stream(ctx, ctx->stream);
    if (st != GDCA_OK) {
        gdca_ctx_destroy(ctx);
        *out = nullptr;
    }
    return st;
}

gdca_status gdca_ctx_create_peer(gdca_ctx *leader, gdca_ctx **out)
{
    if (!leader || !out) return GDCA_EINVAL;
    gdca_ctx *ctx = leader;
    HIPCHK(hipSetDevice(leader->device));
    if (!leader->gate) {
        gdca_gate *g = (gdca_gate *)calloc(1, sizeof(gdca_gate));
        if (!g) return GDCA_ENOMEM;
        for (int i = 0; i < 4; ++i) HIPCHK(hipEventCreateWithFlags(&g->ev[i], hipEventDisableTiming));
        g->refs = 1;
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if (hipStreamCreateWithPriority(&g->batch_stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) g->batch_stream = nullptr;
        leader->gate = g;
    }
    const bool new_gate = leader->gate->refs == 1;
    gdca_status st = gdca_ctx_create(leader->device, out);
    if (st != GDCA_OK) return st;
    (*out)->gate = leader->gate;
    leader->gate->refs += 1;
    if (new_gate && leader->gate->batch_stream) {  // (the pipeline's own stream too)
        st = warm_stream(*out, leader->gate->batch_stream);
        if (st != GDCA_OK) {
            gdca_ctx_destroy(*out);
            *out = nullptr;
        }
    }
    return st;
}

gdca_status gdca_ctx_destroy(gdca_ctx *ctx)
{
    if (!ctx) return GDCA_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream || ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    gdca_buf *bufs[] = {&ctx->Zt, &ctx->Zp, &ctx->hist, &ctx->Zb, &ctx->hcnt, &ctx->nk, &ctx->W, &ctx->Wfix, &ctx->Pifix,
                        &ctx->Pipc, &ctx->A, &ctx->G, &ctx->H, &ctx->P, &ctx->Sg, &ctx->Dblk, &ctx->Ld,
                        &ctx->Tws, &ctx->colsum, &ctx->sc, &ctx->normws, &ctx->C2, &ctx->B0, &ctx->Rt, &ctx->Wd, &ctx->rankws, &ctx->hcand, &ctx->himg,
                        &ctx->Pij, &ctx->sc_front, &ctx->keep, &ctx->Xg, &ctx->Epart, &ctx->gpart, &ctx->gvec,
                        &ctx->PXa, &ctx->PXb, &ctx->PXpad, &ctx->PEab, &ctx->PT, &ctx->PBtab, &ctx->PBitems, &ctx->PBE,
                        &ctx->LOa, &ctx->LOb, &ctx->PBN,
                        &ctx->IPAws, &ctx->IPAcnt, &ctx->IPAZ, &ctx->IPAsel, &ctx->IPAm, &ctx->IPAg, &ctx->IPAprev, &ctx->IPAsp, &ctx->DMd, &ctx->SMst, &ctx->TMst, &ctx->TMx, &ctx->BMws, &ctx->BMred, &ctx->PLMv, &ctx->PLMws,
                        &ctx->AISst, &ctx->AISx, &ctx->AISb};
    for (gdca_buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    ctx->staging.release();
    if (ctx->gate && --ctx->gate->refs == 0) {
        for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ctx->gate->ev[i]);
        if (ctx->gate->batch_stream) {
            (void)hipStreamSynchronize(ctx->gate->batch_stream);
            (void)hipStreamDestroy(ctx->gate->batch_stream);
        }
        free(ctx->gate);
    }
    for (hipEvent_t e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->item0_host) (void)hipHostFree(ctx->item0_host);
    if (ctx->ev_batch) (void)hipEventDestroy(ctx->ev_batch);
    if (ctx->ev_upload) (void)hipEventDestroy(ctx->ev_upload);
    if (ctx->sc_host) (void)hipHostFree(ctx->sc_host);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    free(ctx);
    return GDCA_OK;
}

gdca_status gdca_ctx_synchronize(gdca_ctx *ctx)
{
    if (!ctx) return GDCA_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

const char *gdca_last_error(gdca_ctx *ctx)
{
    return ctx ? ctx->err : "null context";
}

gdca_status gdca_ctx_set_timing(gdca_ctx *ctx, int32_t enabled)
{
    if (!ctx) return GDCA_EINVAL;
    ctx->timing = enabled != 0;
    return GDCA_OK;
}

gdca_status gdca_ctx_set_option(gdca_ctx *ctx, const char *key, const char *value)
{
    if (!ctx) return GDCA_EINVAL;
    if (!key || !value) return fail(ctx, GDCA_EINVAL, "null option key or value");
    if (!gdca_tuning_set(&ctx->tune, key, value)) return fail(ctx, GDCA_EINVAL, "unknown option or unusable value: %s=%s", key, value);
    return GDCA_OK;
}

}  // extern "C"

// ---- the timeline of a run: every gdca_stats.ms_* is the time between two named boundaries (gdca_boundary) ----------------------------
// A timed run marks its boundaries with ONE clock, fixed when it is enqueued: HIP events of its context, or -- a member of a batch
// whose kernels go out as batched grids -- device time stamps written by kernels of the batch (one launch stamps all members).  Only
// an inverse launch of its own is bracketed by events inside a stamped run too.  An untimed run, and the operator-level entries
// (begin() closes the timeline), mark nothing.
static gdca_status open_timeline(gdca_ctx *ctx, bool timed, bool stamped)
{
    gdca_pending &r = ctx->pend;
    r.timed = timed;
    r.stamped = stamped;
    r.ev_marks = r.stamp_marks = 0;
    for (int t = 0; timed && t < T_COUNT; ++t)
        if (!ctx->ev[t]) HIPCHK(hipEventCreate(&ctx->ev[t]));
    return GDCA_OK;
}

static void note_mark(gdca_pending &r, gdca_boundary t, bool stamp)
{
    (stamp ? r.stamp_marks : r.ev_marks) |= 1u << t;
    (stamp ? r.ev_marks : r.stamp_marks) &= ~(1u << t);
}

// boundary t of the context's run, here on its stream.  own_launch: by an event whatever the run's clock
static gdca_status mark(gdca_ctx *ctx, gdca_boundary t, bool own_launch = false)
{
    gdca_pending &r = ctx->pend;
    if (!r.timed) return GDCA_OK;
    const bool stamp = r.stamped && !own_launch;
    if (stamp)
        gdca_launch_stamp(ctx->stream, (gdca_dev_scalars *)ctx->sc.p, t, T_NONE);
    else
        HIPCHK(hipEventRecord(ctx->ev[t], ctx->stream));
    note_mark(r, t, stamp);
    return GDCA_OK;
}

// boundaries a and b, one instant on stream s, of all K members of a merged launch (all timed): two events of ITS OWN for every
// member -- members may be collected, enqueued again or destroyed in any order, and a collect must never read another context's events
//  -- or, stamps: one launch of the batched k_stamp for all of them (2 launches around a merged sweep instead of 4 K records)
static gdca_status mark_members(hipStream_t s, gdca_ctx *const *mem, int K, gdca_boundary a, gdca_boundary b, bool stamps)
{
    gdca_ctx *ctx = mem[0];
    if (stamps) {
        gdca_recorder *&act = gdca_recorder::active();
        gdca_recorder *outer = act;
        if (outer) (void)outer->flush();
        gdca_recorder rec;
        rec.begin(s, K);
        for (int k = 0; k < K; ++k) {
            rec.member(k);
            gdca_launch_stamp(s, (gdca_dev_scalars *)mem[k]->sc.p, a, b);
        }
        (void)rec.end();
        act = outer;
    } else
        for (int k = 0; k < K; ++k) {
            HIPCHK(hipEventRecord(mem[k]->ev[a], s));
            HIPCHK(hipEventRecord(mem[k]->ev[b], s));
        }
    for (int k = 0; k < K; ++k) {
        note_mark(mem[k]->pend, a, stamps);
        note_mark(mem[k]->pend, b, stamps);
    }
    return GDCA_OK;
}

// the two events the sweep launchers record themselves, behind k_sweep_prep (null: an untimed run)
static void sweep_events(gdca_ctx *ctx, hipEvent_t *begin, hipEvent_t *end)
{
    const bool timed = ctx->pend.timed;
    *begin = timed ? ctx->ev[T_SWEEP_BEGIN] : nullptr;
    *end = timed ? ctx->ev[T_SWEEP_END] : nullptr;
    note_mark(ctx->pend, T_SWEEP_BEGIN, false);
    note_mark(ctx->pend, T_SWEEP_END, false);
}

// milliseconds of device time from boundary a to boundary b of the collected run: both marked by the same clock, 0 otherwise
static double elapsed(const gdca_ctx *ctx, gdca_boundary a, gdca_boundary b, bool *failed)
{
    const gdca_pending &r = ctx->pend;
    const unsigned both = 1u << a | 1u << b;
    if (!r.timed) return 0.0;
    if ((r.stamp_marks & both) == both) return (double)(long long)(ctx->sc_host->stamp[b] - ctx->sc_host->stamp[a]) * 1e-5;
    if ((r.ev_marks & both) != both) return 0.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]) != hipSuccess) *failed = true;
    return ms;
}

// a pipeline's gate: the stream waits for the inverse that went through it last; the inverse just enqueued becomes that one
static hipError_t gate_wait(const gdca_gate *g, hipStream_t s)
{
    return g->armed ? hipStreamWaitEvent(s, g->ev[g->last], 0) : hipSuccess;
}

static hipError_t gate_pass(gdca_gate *g, hipStream_t s)
{
    const hipError_t e = hipEventRecord(g->ev[g->next], s);
    if (e != hipSuccess) return e;
    g->last = g->next;
    g->next = (g->next + 1) & 3;
    g->armed = 1;
    return hipSuccess;
}

// a member's failure as the LEADER's last error (the caller of a batch entry reads the leader's)
static gdca_status member_error(gdca_ctx *lead, gdca_ctx *m, int k, gdca_status st)
{
    if (k > 0 && m != lead && m->err[0]) {
        char msg[sizeof(lead->err)];
        snprintf(msg, sizeof(msg), "member %d: %.400s", k, m->err);
        memcpy(lead->err, msg, sizeof(msg));
    }
    return st;
}

// The host buffer of an upload just enqueued on ctx->stream may be reused by the caller: true at once for pageable memory (the copy
// is staged before hipMemcpyAsync returns), a DMA still in flight for pinned or registered memory -- wait for it (an event right
// behind the copy; the stream of a context that is not pending holds nothing else)
static gdca_status upload_done(gdca_ctx *ctx)
{
    HIPCHK(hipEventRecord(ctx->ev_upload, ctx->stream));
    HIPCHK(hipEventSynchronize(ctx->ev_upload));
    return GDCA_OK;
}

static double inverse_flops_model(double n)
{
    return (n * n * n / 3.0 + n * n / 2.0 + n / 6.0) + (2.0 * n * n * n / 3.0 + n * n / 2.0 + 5.0 * n / 6.0);
}

static int round_up(int x, int m)
{
    return (x + m - 1) / m * m;
}

// stage 1+2: theta, threshold, neighbour counts, W, Wfix, Meff  (all on device)
static gdca_status weights_stage(gdca_ctx *ctx, const int8_t *Zd, int N, int M, int q, double theta_in, int fixed_thresh,
                                 bool want_theta_only)
{
    hipStream_t s = ctx->stream;
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    CHK(ensure(ctx, ctx->hist, gdca_column_hist_bytes(N, M)));
    if (fixed_thresh >= 0) {
        gdca_launch_set_thresh(s, sc, fixed_thresh);
    } else {
        if (theta_in < 0.0) gdca_launch_column_hist(s, Zd, (uint32_t *)ctx->hist.p, N, M);
        gdca_launch_theta_finalize(s, (const uint32_t *)ctx->hist.p, N, M, theta_in, sc);
    }
    CHK(check_launch(ctx, "theta"));
    CHK(mark(ctx, T_THETA));
    if (want_theta_only) return GDCA_OK;

    const int Mt = (M + GDCA_HTILE - 1) / GDCA_HTILE;
    CHK(ensure(ctx, ctx->Zb, gdca_bitplane_bytes(N, M)));
    CHK(ensure(ctx, ctx->hcnt, (size_t)Mt * GDCA_HTILE * sizeof(int32_t)));
    if (!ctx->tune.force_fallback && ctx->tune.hamming_mode != 0) CHK(ensure(ctx, ctx->hcand, gdca_hamming_cand_cap(M) * 8));
    // (the consensus form's image, N / 2 bytes per sequence: where the option asks for that form, and where the automatic rule may
    // choose it -- gdca_hamming_form.h: small families are not even probed for it)
    const bool fp4 = !ctx->tune.force_fallback && (ctx->tune.hamming_mode == 2 || (ctx->tune.hamming_mode < 0 && gdca_hamming_consensus_gate(N, M)));
    if (fp4) CHK(ensure(ctx, ctx->himg, gdca_fp4_image_bytes(N, M)));
    CHK(ensure(ctx, ctx->nk, (size_t)M * sizeof(int32_t)));
    CHK(ensure(ctx, ctx->W, (size_t)M * sizeof(double)));
    CHK(ensure(ctx, ctx->Wfix, (size_t)M * sizeof(unsigned long long)));
    gdca_fill_async(s, ctx->hcnt.p, 0, (size_t)Mt * GDCA_HTILE * sizeof(int32_t));
    gdca_launch_bitplane_pack(s, Zd, (uint32_t *)ctx->Zb.p, N, M, q, sc);  // (also the symbol-range check)
    // option GDCA_FORCE_FALLBACK: the independent byte-compare kernel instead of the bit-sliced one -- the analogue of
    // DCAUTILS_FORCE_FALLBACK in the reference's tests (test/runtests.jl:78-86)
    if (ctx->tune.force_fallback) {
        gdca_launch_hamming_fallback(s, Zd, (int32_t *)ctx->hcnt.p, N, M, sc);
    } else {
        if (fp4) {
            // sigma comes from the column histogram, which so far only theta = :auto has counted
            if (!(fixed_thresh < 0 && theta_in < 0.0)) gdca_launch_column_hist(s, Zd, (uint32_t *)ctx->hist.p, N, M);
            gdca_launch_hamming_fp4_image(s, Zd, (const uint32_t *)ctx->hist.p, ctx->himg.p, N, M);
        }
        gdca_launch_hamming(s, (const uint32_t *)ctx->Zb.p, Zd, (int32_t *)ctx->hcnt.p, N, M, sc, ctx->tune.hamming_mode, ctx->hcand.p, fp4 ? ctx->himg.p : nullptr, ctx->tune.ham_cut);
    }
    gdca_launch_weights(s, (const int32_t *)ctx->hcnt.p, M, gdca_fix_shift(M), (int32_t *)ctx->nk.p,
                        (double *)ctx->W.p, (unsigned long long *)ctx->Wfix.p);
    // (Meff: an exact integer sum by one workgroup, microseconds.  Rounds 1-4 summed left to right in f64 -- 0.3 ms of dependent adds at
    // M = 50 000 -- on a side stream of the context, joined before the first consumer.)
    gdca_launch_meff(s, (const double *)ctx->W.p, M, sc);
    return check_launch(ctx, "weights");
}

// stage 3: Pi, pair tallies.  mode 0 -> Pij_true (ld) ; mode 1 -> covariance (ld)
// want_norm1 (mode 1): the fused path's first build -- sc->pi_max, and sc->mat_norm1 = ||C||_1 where the screen needs it (k_cov_norm1)
static gdca_status tally_stage(gdca_ctx *ctx, const int8_t *Zd, int N, int M, int q, const double *Meff_dev, double pc,
                               int mode, double *Pi_true_out, double *out, size_t ld, bool want_norm1 = false)
{
    hipStream_t s = ctx->stream;
    const int sdim = q - 1, n = N * sdim;
    const int shift = gdca_fix_shift(M);
    const int TJ = gdca_tally_tj(q, ctx->tune.tally_tj);
    const bool skip = gdca_tally_skip(q, TJ, ctx->tune.tally_skip, M);
    const size_t keep_list = (size_t)N * M * sizeof(uint32_t);  // then keep_n (N int), sigma (N bytes)
    if (skip) CHK(ensure(ctx, ctx->keep, keep_list + (size_t)N * sizeof(int) + N));
    CHK(ensure(ctx, ctx->Zt, (size_t)N * M + 3));  // (k_pi_keep reads whole aligned dwords)
    CHK(ensure(ctx, ctx->Zp, (size_t)round_up(N, 64) * M + 64));
    CHK(ensure(ctx, ctx->Pifix, (size_t)N * 32 * sizeof(unsigned long long)));
    CHK(ensure(ctx, ctx->Pipc, (size_t)n * sizeof(double)));
    uint32_t *keep = skip ? (uint32_t *)ctx->keep.p : nullptr;
    int *keep_n = skip ? (int *)((char *)ctx->keep.p + keep_list) : nullptr;
    uint8_t *sigma = skip ? (uint8_t *)(keep_n + N) : nullptr;
    gdca_launch_relayout(s, Zd, (int8_t *)ctx->Zt.p, (int8_t *)ctx->Zp.p, N, M, TJ);
    // single-site sums and (TALLY_SKIP) the lists of the pair tally: one kernel over Zt, every output stored by its one owner
    gdca_launch_pi_keep(s, (const int8_t *)ctx->Zt.p, (const unsigned long long *)ctx->Wfix.p, (unsigned long long *)ctx->Pifix.p, keep, keep_n,
                        sigma, N, M, q, (gdca_dev_scalars *)ctx->sc.p);
    gdca_launch_pi_finalize(s, (const unsigned long long *)ctx->Pifix.p, N, q, shift, Meff_dev, pc, Pi_true_out,
                            (double *)ctx->Pipc.p, want_norm1 ? &((gdca_dev_scalars *)ctx->sc.p)->pi_max : nullptr);
    if (want_norm1) CHK(mark(ctx, T_TALLY_BEGIN));  // (the fused path's first build: its own device time, gdca_stats.ms_pair_tally)
    gdca_launch_pair_tally(s, (const int8_t *)ctx->Zp.p, (const int8_t *)ctx->Zt.p,
                           (const unsigned long long *)ctx->Wfix.p, N, M, q, shift, Meff_dev, pc,
                           (const double *)ctx->Pipc.p, mode, out, ld, TJ, keep, keep_n, sigma,
                           (const unsigned long long *)ctx->Pifix.p);
    if (want_norm1) CHK(mark(ctx, T_TALLY_END));
    // ||C||_1 for the refinement screen, where the bound that costs nothing (2 N pi_max) does not settle it (k_cov_norm1)
    // (not even launched where the answer is known on the host: pi_max <= (1 - pc) + pc / q whatever the alignment)
    if (want_norm1 && !gdca_norm1_settled(N, q, pc, ctx->tune.refine, ctx->tune.refine_cond))
        gdca_launch_cov_norm1(s, out, ld, N, q, pc, ctx->tune.refine_cond, (gdca_dev_scalars *)ctx->sc.p, ctx->tune.refine == 1);
    return check_launch(ctx, "tally");
}

// the workspace of one inverse: 2 x 4 panels G and H (pivot groups of up to four blocks, double-buffered by group parity), one
// 128 x 128 pivot inverse, four 512 x 512 scratch matrices for a group's diagonal super-block, the sweep's flags and item table
static gdca_status inverse_job(gdca_ctx *ctx, int n, int n_pad, gdca_inverse_job *job)
{
    const size_t pbytes = (size_t)n_pad * GDCA_TILE * sizeof(double);
    const int nblk = n_pad / GDCA_TILE;
    const size_t sg = (size_t)4 * GDCA_TILE * 4 * GDCA_TILE * sizeof(double);
    const size_t fbytes = gdca_inverse_flag_bytes(n_pad);
    CHK(ensure(ctx, ctx->G, (size_t)8 * pbytes));
    CHK(ensure(ctx, ctx->H, (size_t)8 * pbytes));
    CHK(ensure(ctx, ctx->P, (size_t)GDCA_TILE * GDCA_TILE * sizeof(double)));
    const int item_ints = gdca_sweep::table_ints_max(nblk);  // the sweep's item table, whatever groups it picks
    const size_t piv_off = (4 * sg + fbytes + (size_t)item_ints * sizeof(int) + 15) & ~(size_t)15;
    CHK(ensure(ctx, ctx->Sg, piv_off + (size_t)n_pad * sizeof(double)));
    if (ctx->item0_cap < item_ints) {
        if (ctx->item0_host) HIPCHK(hipHostFree(ctx->item0_host));
        ctx->item0_host = nullptr;
        ctx->item0_cap = 0;
        HIPCHK(hipHostMalloc((void **)&ctx->item0_host, (size_t)item_ints * sizeof(int), hipHostMallocDefault));
        ctx->item0_cap = item_ints;
    }
    gdca_inverse_ws &ws = job->ws;
    for (int w = 0; w < 8; ++w) {
        ws.G[w] = (double *)((char *)ctx->G.p + (size_t)w * pbytes);
        ws.H[w] = (double *)((char *)ctx->H.p + (size_t)w * pbytes);
    }
    ws.P = (double *)ctx->P.p;
    ws.Sg[0] = (double *)ctx->Sg.p;
    ws.Sg[1] = (double *)((char *)ctx->Sg.p + sg);
    ws.Pg[0] = (double *)((char *)ctx->Sg.p + 2 * sg);
    ws.Pg[1] = (double *)((char *)ctx->Sg.p + 3 * sg);
    ws.flags = (unsigned *)((char *)ctx->Sg.p + 4 * sg);
    ws.flags_bytes = fbytes;
    ws.item0_dev = (int *)((char *)ctx->Sg.p + 4 * sg + fbytes);
    ws.item0_host = ctx->item0_host;
    ws.piv = ctx->piv = (double *)((char *)ctx->Sg.p + piv_off);
    ctx->ld.count = 0;  // (an inverse is on its way: the last one's log det is history)
    ctx->ld.chol = false;
    {
        void *dp = nullptr;
        ws.item0_host_dev = hipHostGetDevicePointer(&dp, ctx->item0_host, 0) == hipSuccess ? (const int *)dp : nullptr;
    }
    ws.update_cus = ctx->ncu;
    job->A = (double *)ctx->A.p;
    job->n_pad = n_pad;
    job->n_real = n;
    job->sc = (gdca_dev_scalars *)ctx->sc.p;
    job->tune = &ctx->tune;
    job->doomed = (ctx->tune.sweep_debug & 32) != 0 && ctx->pend.at.attempt == 0;
    return GDCA_OK;
}

static gdca_status poison_inverse_ws(gdca_ctx *ctx, hipStream_t s)
{
    HIPCHK(hipMemsetAsync(ctx->G.p, 0xFF, ctx->G.cap, s));
    HIPCHK(hipMemsetAsync(ctx->H.p, 0xFF, ctx->H.cap, s));
    HIPCHK(hipMemsetAsync(ctx->P.p, 0xFF, ctx->P.cap, s));
    HIPCHK(hipMemsetAsync(ctx->Sg.p, 0xFF, (size_t)4 * 4 * GDCA_TILE * 4 * GDCA_TILE * sizeof(double), s));
    return GDCA_OK;
}

static gdca_status inverse_stage(gdca_ctx *ctx, int n, int n_pad, double *upd_flops)
{
    gdca_inverse_job job;
    CHK(inverse_job(ctx, n, n_pad, &job));
    hipEvent_t sweep_begin, sweep_end;
    sweep_events(ctx, &sweep_begin, &sweep_end);
    // tests (option SWEEP_DEBUG): bit 4 = the panel / scratch buffers are poisoned with NaNs first (an item that reads a buffer
    // before its producer wrote it can then not pass on the leftovers of an earlier, identical run); bit 3 = the merged kernel
    // carries this single inverse
    if (ctx->tune.sweep_debug & 16) CHK(poison_inverse_ws(ctx, ctx->stream));
    if (ctx->tune.sweep_debug & 8) {
        double fl = 0.0;
        gdca_launch_spd_inverse_merged(ctx->stream, &job, 1, sweep_begin, sweep_end, &fl);
        if (upd_flops) *upd_flops = fl;
        return check_launch(ctx, "spd_inverse_merged");
    }
    gdca_launch_spd_inverse(ctx->stream, job, sweep_begin, sweep_end, upd_flops);
    return check_launch(ctx, "spd_inverse");
}

// log det of the matrix just inverted into sc->logdet, from the pivots the sweep (or the Cholesky fallback) left in ctx->piv: one small
// launch behind the inverse on its stream (k_logdet.hip)
static gdca_status logdet_stage(gdca_ctx *ctx, int n)
{
    gdca_launch_logdet(ctx->stream, ctx->piv, n, (gdca_dev_scalars *)ctx->sc.p);
    return check_launch(ctx, "logdet");
}

// ... and, the scalars fetched, kept as the context's last (member k of a gdca_run_multi call; everything else has one member)
static void note_logdet(gdca_ctx *ctx, int k = 0)
{
    const gdca_dev_scalars &h = *ctx->sc_host;
    ctx->ld.val[k] = h.info == 0 && !h.bad_symbol ? h.logdet : (double)NAN;
    ctx->ld.src[k] = ctx->ld.chol ? 1 : 0;
    ctx->ld.count = k + 1;
}

// What the energies and the mutation scan open with: the K sequences X (N x K) packed into ctx->Xg (illegal bytes: sc->bad_symbol
// bit 2), g = mJ Pi in ctx->gvec and c0 = Pi' g behind it.
static gdca_status g_room(gdca_ctx *ctx, int n)
{
    const int nb = gdca_energy_gblocks(n);
    CHK(ensure(ctx, ctx->gpart, (size_t)nb * nb * 64 * sizeof(double)));
    return ensure(ctx, ctx->gvec, ((size_t)n + 1) * sizeof(double));
}

// g = mJ Pi of the model m into ctx->gvec, c0 behind it (g_room first): the one g of the library -- the energies', the mutation
// stage's and the Potts warm start's (gdca_potts_from_gaussian_dev)
static void g_launch(gdca_ctx *ctx, const gdca_model &m)
{
    const int n = m.N * (m.q - 1);
    double *g = (double *)ctx->gvec.p;
    gdca_launch_energy_g(ctx->stream, m.A, m.ld, m.sign, n, m.Pi, (double *)ctx->gpart.p, g, g + n);
}

static gdca_status pack_and_g(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, size_t stride = 0)
{
    CHK(ensure(ctx, ctx->Xg, (size_t)gdca_energy_blocks(m.N) * K * sizeof(uint32_t)));
    CHK(g_room(ctx, m.N * (m.q - 1)));
    gdca_launch_energy_pack(ctx->stream, X_dev, stride ? stride : (size_t)m.N, m.N, K, m.q, (uint32_t *)ctx->Xg.p, (gdca_dev_scalars *)ctx->sc.p);
    g_launch(ctx, m);
    return GDCA_OK;
}

// E[K] = 1/2 (x - Pi)' mJ (x - Pi) of the K sequences X (N x K) under the model m.  Illegal bytes of X: sc->bad_symbol, GDCA_BAD_SEQUENCE.
// stride != 0: sequence k starts at X_dev + k * stride (a range of the sites of longer sequences)
static gdca_status energy_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, double *E_dev, size_t stride = 0)
{
    const int sdim = m.q - 1, n = m.N * sdim;
    const int Kc = gdca_energy_chunk(m.N, K, ctx->tune.energy_chunk);
    CHK(ensure(ctx, ctx->Epart, (size_t)gdca_energy_blocks(m.N) * Kc * sizeof(double)));
    CHK(pack_and_g(ctx, m, X_dev, K, stride));
    const double *g = (const double *)ctx->gvec.p;
    for (int k0 = 0; k0 < K; k0 += Kc)
        HIPCHK(gdca_launch_energy_rows(ctx->stream, m.A, m.ld, m.sign, g, g + n, (const uint32_t *)ctx->Xg.p, m.N, sdim, K, k0,
                                       std::min(Kc, K - k0), (double *)ctx->Epart.p, E_dev, ctx->ncu));
    return check_launch(ctx, "energies");
}

// E[a + KA * b] of the KA x KB pairings a (+) b across the split (k_pair_energy.hip) under the model m.  XA / XB point at the first
// site of sequence 0's half; sequence k's starts strideA / strideB bytes on (so the columns of an alignment serve as they lie).
// what = GDCA_PAIR_ENERGY: the marginal energies through energy_stage on the gap-padded halves (m.Pi needed), combined in the gather
// kernel's epilogue; GDCA_PAIR_COUPLING: R alone, no g.  Illegal bytes: sc->bad_symbol, GDCA_BAD_SEQUENCE.
// lo != nullptr (what = GDCA_PAIR_ENERGY): the log-odds ((EmA[a] + EmB[b]) - E[a, b]) + I in the place of the energy (the gather's LO instances).
// blk != nullptr: only the pairings inside the species of species-sorted sequences, E packed block by block (include/gdca.h, partner
// matching) -- the pack, the pad, the marginal energies and the fold are the same calls; the gather goes by blk's work list.
// what the pair stage makes of its sequences alone, whatever the model: the packed symbols of the two halves (ctx->PXa, ctx->PXb;
// illegal bytes: sc->bad_symbol, GDCA_BAD_SEQUENCE) and, for the energy, the gap-padded halves (ctx->PXpad)
static gdca_status pair_pack(gdca_ctx *ctx, int N, int q, int split, const int8_t *XA, size_t strideA, int KA, const int8_t *XB, size_t strideB,
                             int KB, int what)
{
    hipStream_t s = ctx->stream;
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    CHK(ensure(ctx, ctx->PXa, (size_t)gdca_energy_blocks(split) * KA * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->PXb, (size_t)gdca_energy_blocks(N - split) * KB * sizeof(uint32_t)));
    gdca_launch_energy_pack(s, XA, strideA, split, KA, q, (uint32_t *)ctx->PXa.p, sc);
    gdca_launch_energy_pack(s, XB, strideB, N - split, KB, q, (uint32_t *)ctx->PXb.p, sc);
    if (what == GDCA_PAIR_ENERGY) {
        CHK(ensure(ctx, ctx->PXpad, (size_t)N * ((size_t)KA + (size_t)KB)));
        gdca_launch_pair_pad(s, XA, strideA, XB, strideB, N, split, KA, KB, q, (int8_t *)ctx->PXpad.p);
    }
    return GDCA_OK;
}

// packed: pair_pack has run on these sequences already and nothing has touched its three buffers since (the rounds of
// gdca_run_partner_ipa: the pools do not change from round to round)
static gdca_status pair_stage(gdca_ctx *ctx, const gdca_model &m, int split, const int8_t *XA, size_t strideA, int KA, const int8_t *XB,
                              size_t strideB, int KB, int what, double *E_dev, const pair_blocks *blk = nullptr, bool packed = false,
                              const gdca_logodds_terms *lo = nullptr)
{
    hipStream_t s = ctx->stream;
    const int N = m.N, q = m.q, sdim = q - 1, n = N * sdim, nB = (N - split) * sdim;
    if (!packed) CHK(pair_pack(ctx, N, q, split, XA, strideA, KA, XB, strideB, KB, what));
    const double *EAB = nullptr, *c0 = nullptr;
    if (what == GDCA_PAIR_ENERGY) {
        CHK(ensure(ctx, ctx->PEab, ((size_t)KA + (size_t)KB) * sizeof(double)));
        CHK(energy_stage(ctx, m, (const int8_t *)ctx->PXpad.p, KA + KB, (double *)ctx->PEab.p));
        EAB = (const double *)ctx->PEab.p;
        c0 = (const double *)ctx->gvec.p + n;
    }
    const int Ac = blk ? blk->Ac : gdca_pair_chunk(nB, KA, ctx->tune.pair_chunk);
    CHK(ensure(ctx, ctx->PT, (size_t)Ac * nB * sizeof(double)));
    for (int a0 = 0, c = 0; a0 < KA; a0 += Ac, ++c) {
        if (blk)
            HIPCHK(gdca_launch_pair_chunk_blocked(s, m.A, m.ld, m.sign, (const uint32_t *)ctx->PXa.p, (const uint32_t *)ctx->PXb.p, N, split, sdim,
                                                  KA, KB, a0, std::min(Ac, KA - a0), (double *)ctx->PT.p, EAB, c0, E_dev,
                                                  blk->items + 4 * blk->first[c], blk->first[c + 1] - blk->first[c], blk->eoff, blk->offA,
                                                  blk->offB, ctx->ncu, lo));
        else
            HIPCHK(gdca_launch_pair_chunk(s, m.A, m.ld, m.sign, (const uint32_t *)ctx->PXa.p, (const uint32_t *)ctx->PXb.p, N, split, sdim, KA, KB,
                                          a0, std::min(Ac, KA - a0), (double *)ctx->PT.p, EAB, c0, E_dev, ctx->ncu, lo));
    }
    return check_launch(ctx, blk ? "blocked pair energies" : "pair energies");
}

// match / gap of the assignment inside every block of the packed cost matrix E_dev (k_assign.hip)
static gdca_status assign_stage(gdca_ctx *ctx, const double *E_dev, const pair_blocks &blk, int32_t *match_dev, double *gap_dev)
{
    HIPCHK(gdca_launch_assign_blocks(ctx->stream, E_dev, blk.eoff, blk.offA, blk.offB, blk.S, blk.kmax, match_dev, gap_dev));
    return check_launch(ctx, "assignment");
}

// D[(b - 1) + q (i + N k)]: the site potentials V (what = GDCA_MUT_POTENTIAL) or the energy changes dE (GDCA_MUT_DELTA) of every single
// substitution of the K sequences X (N x K) (k_mutation.hip) under the model m.  Illegal bytes of X: sc->bad_symbol, GDCA_BAD_SEQUENCE.
static gdca_status mutation_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, int what, double *D_dev)
{
    CHK(pack_and_g(ctx, m, X_dev, K));
    HIPCHK(gdca_launch_mutation_scan(ctx->stream, m.A, m.ld, m.sign, (const double *)ctx->gvec.p, (const uint32_t *)ctx->Xg.p, m.N, m.q - 1, K,
                                     what, D_dev, ctx->ncu));
    return check_launch(ctx, "mutation scan");
}

// The double-mutant read-outs (k_epistasis.hip) of the K sequences X (N x K) under the model m: dE of every single substitution into
// ctx->DMd first (the mutation stage), then -- muts == nullptr -- the maps Emin / code / epi (N x N x K; each may be nullptr) over the
// block lower triangle, or the L listed double mutants (5 x L records) into out.  Illegal bytes of X: sc->bad_symbol, GDCA_BAD_SEQUENCE; a record
// out of range: bit 4.
static gdca_status double_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, double *Emin_dev, int32_t *code_dev,
                                double *epi_dev, const int32_t *muts_dev, int L, double *out_dev)
{
    CHK(ensure(ctx, ctx->DMd, (size_t)m.q * (size_t)m.N * (size_t)K * sizeof(double)));
    CHK(mutation_stage(ctx, m, X_dev, K, GDCA_MUT_DELTA, (double *)ctx->DMd.p));
    if (muts_dev) {
        gdca_launch_double_mutants(ctx->stream, m.A, m.ld, m.sign, (const uint32_t *)ctx->Xg.p, (const double *)ctx->DMd.p, muts_dev, L, m.N,
                                   m.q - 1, K, out_dev, (gdca_dev_scalars *)ctx->sc.p);
        return check_launch(ctx, "double mutants");
    }
    HIPCHK(gdca_launch_double_mutant_scan(ctx->stream, m.A, m.ld, m.sign, (const uint32_t *)ctx->Xg.p, (const double *)ctx->DMd.p, m.N, m.q - 1,
                                          K, Emin_dev, code_dev, epi_dev, ctx->tune.epi_generic != 0));
    return check_launch(ctx, "double-mutant scan");
}

// Where the walk keeps a sequence's table (option WALK_TABLE): in LDS where it fits, unless HBM is asked for; an error: LDS asked for
// and the table does not fit
static gdca_status walk_placement(gdca_ctx *ctx, int N, int q, bool *in_lds)
{
    const bool fits = gdca_walk_table_fits(N, q);
    *in_lds = ctx->tune.walk_table == 2 ? false : fits;
    if (!fits && ctx->tune.walk_table == 1) return fail(ctx, GDCA_EINVAL, "WALK_TABLE = lds: the table does not fit into LDS");
    return GDCA_OK;
}

// What the walk and the chains open with: the tables' placement, their room -- *V as the caller gave it or, where that is nullptr,
// ctx->DMd sized for the K sequences X (N x K) --, and the sequences' site potentials in it through the mutation stage (ctx->Xg: the
// K starts packed, as the first launch reads them)
static gdca_status table_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, double **V, bool *in_lds)
{
    CHK(walk_placement(ctx, m.N, m.q, in_lds));
    if (!*V) {
        CHK(ensure(ctx, ctx->DMd, (size_t)m.q * (size_t)m.N * (size_t)K * sizeof(double)));
        *V = (double *)ctx->DMd.p;
    }
    return mutation_stage(ctx, m, X_dev, K, GDCA_MUT_POTENTIAL, *V);
}

// the end of the chains' launch that starts at proposal t0: at most SAMPLE_CHUNK proposals
static int chunk_end(const gdca_ctx *ctx, int t0, int n_steps)
{
    const int chunk = ctx->tune.sample_chunk > 0 ? ctx->tune.sample_chunk : GDCA_SAMPLE_CHUNK_RULE;
    return n_steps - t0 > chunk ? t0 + chunk : n_steps;
}

// The greedy walk (k_walk.hip) of the K sequences X (N x K) under the model m: their site potentials through the mutation stage into
// w.V -- or, where the caller does not want the final tables, into ctx->DMd --, then one workgroup a sequence walks its table, in LDS
// or in place.  Illegal bytes of X: sc->bad_symbol, GDCA_BAD_SEQUENCE (they count as gaps: nothing is indexed with them).
static gdca_status walk_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, const walk_request &w)
{
    bool in_lds = false;
    double *V = w.V;
    CHK(table_stage(ctx, m, X_dev, K, &V, &in_lds));
    HIPCHK(gdca_launch_greedy_walk(ctx->stream, m.A, m.ld, m.sign, (const uint32_t *)ctx->Xg.p, m.N, m.q - 1, K, w.mask, w.flags, w.min_gain,
                                   w.max_steps, V, in_lds, w.V != nullptr, w.Xout, w.steps, w.dE_sum, w.path, w.dE_path));
    return check_launch(ctx, "greedy walk");
}

// The Metropolis chains (k_sample.hip) from the K sequences X (N x K) under the model m: the start tables through the mutation stage
// into r.V -- or into ctx->DMd --, placed as the walk places them, then the proposals in launches of at most SAMPLE_CHUNK; between two
// launches a chain lives in its table, in ctx->SMst and in `accepted`.  Illegal bytes of X: as the walk's.
static gdca_status sample_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, const sample_request &r)
{
    bool in_lds = false;
    double *V = r.V;
    CHK(ensure(ctx, ctx->SMst, gdca_sample_state_bytes(m.N, K)));
    CHK(table_stage(ctx, m, X_dev, K, &V, &in_lds));
    const int n_steps = r.plan.chain.n_steps();
    for (int t0 = 0; t0 < n_steps;) {
        const int t1 = chunk_end(ctx, t0, n_steps);
        HIPCHK(gdca_launch_sample(ctx->stream, m.A, m.ld, m.sign, (const uint32_t *)ctx->Xg.p, m.N, m.q - 1, K, r.plan, t0, t1, V, in_lds,
                                  ctx->SMst.p));
        t0 = t1;
    }
    return check_launch(ctx, "Metropolis chains");
}

// The replica-exchange chains (k_temper.hip) of K chains of R replicas under the model m, from X_dev: N x R x K, or -- r.fused -- N x K
// replicated into ctx->TMx.  The start tables (the mutation stage, into ctx->DMd: q N K R doubles) and the start energies (the energy
// stage) of the K R replicas as of so many sequences, the maps, then launch by launch: the proposals up to the next round or
// SAMPLE_CHUNK boundary, the round.  The only coupling between replicas is the order of the launches on the stream.
static gdca_status temper_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *X_dev, int K, const temper_request &r)
{
    bool in_lds = false;
    CHK(walk_placement(ctx, m.N, m.q, &in_lds));  // (before anything is enqueued; table_stage asks again)
    const gdca_temper_plan &plan = r.plan;
    const int R = plan.R, G = K * R;
    hipStream_t s = ctx->stream;
    const int8_t *Xr = X_dev;
    if (r.fused) {
        CHK(ensure(ctx, ctx->TMx, (size_t)m.N * (size_t)G));
        gdca_launch_temper_replicate(s, X_dev, m.N, K, R, (int8_t *)ctx->TMx.p);
        Xr = (const int8_t *)ctx->TMx.p;
    }
    CHK(ensure(ctx, ctx->TMst, gdca_temper_state_bytes(m.N, G)));
    void *state = ctx->TMst.p;
    CHK(energy_stage(ctx, m, Xr, G, gdca_temper_E0(state, G)));
    double *V = nullptr;  // (ctx->DMd: q N K R doubles)
    CHK(table_stage(ctx, m, Xr, G, &V, &in_lds));
    gdca_launch_temper_init(s, plan, K, state, (gdca_dev_scalars *)ctx->sc.p);
    const int n_steps = plan.chain.n_steps(), every = plan.swap_every;
    for (int t0 = 0; t0 < n_steps;) {
        const int round_end = (t0 / every + 1) * every;  // (every divides n_steps)
        const int t1 = std::min(round_end, chunk_end(ctx, t0, n_steps));
        HIPCHK(gdca_launch_temper_chain(s, m.A, m.ld, m.sign, (const uint32_t *)ctx->Xg.p, m.N, m.q - 1, K, plan, t0, t1, V, in_lds, state));
        if (t1 == round_end) {
            const int past = t1 - plan.chain.burn;  // a sample point: t1 = burn + (j + 1) stride
            const int js = past > 0 && past % plan.chain.stride == 0 ? past / plan.chain.stride - 1 : -1;
            gdca_launch_temper_round(s, m.N, K, plan, t1 / every - 1, js, state);
        }
        t0 = t1;
    }
    gdca_launch_temper_finish(s, m.N, K, plan, state);
    return check_launch(ctx, "replica-exchange chains");
}

// The annealed chains (k_ais.hip) of K uniform starts over the state space of the template x_dev (nullptr: every site is free) under the
// model m, along the HOST ladder betas[0 .. L]: the ladder into ctx->AISb, the starts into ctx->AISx, their energies (the energy stage)
// and tables (the mutation stage, into ctx->DMd: q N K doubles) as of so many sequences -- temper_stage's pairing --, the proposals in
// launches of at most SAMPLE_CHUNK, the reduction.  Between two launches a chain lives in its table and in ctx->AISst.
static gdca_status ais_stage(gdca_ctx *ctx, const gdca_model &m, const int8_t *x_dev, int K, const double *betas, gdca_ais_plan plan)
{
    bool in_lds = false;
    CHK(walk_placement(ctx, m.N, m.q, &in_lds));  // (before anything is enqueued; table_stage asks again)
    hipStream_t s = ctx->stream;
    CHK(ensure(ctx, ctx->AISb, ((size_t)plan.L + 1) * sizeof(double)));
    CHK(ensure(ctx, ctx->AISx, (size_t)m.N * (size_t)K));
    CHK(ensure(ctx, ctx->AISst, gdca_ais_state_bytes(m.N, K)));
    void *state = ctx->AISst.p;
    int8_t *Xst = (int8_t *)ctx->AISx.p;
    HIPCHK(hipMemcpyAsync(ctx->AISb.p, betas, ((size_t)plan.L + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (the caller's array is free once the call returns, whatever fails below)
    plan.betas = (const double *)ctx->AISb.p;
    gdca_launch_ais_start(s, x_dev, m.N, m.q, K, plan, Xst, state);
    CHK(energy_stage(ctx, m, Xst, K, gdca_ais_E0(state, K)));
    double *V = nullptr;  // (ctx->DMd: q N K doubles)
    CHK(table_stage(ctx, m, Xst, K, &V, &in_lds));
    const int n_steps = plan.chain.n_steps();
    for (int t0 = 0; t0 < n_steps;) {
        const int t1 = chunk_end(ctx, t0, n_steps);
        HIPCHK(gdca_launch_ais(s, m.A, m.ld, m.sign, (const uint32_t *)ctx->Xg.p, m.N, m.q - 1, K, plan, t0, t1, V, in_lds, state));
        t0 = t1;
    }
    gdca_launch_ais_reduce(s, K, (plan.chain.flags & GDCA_SAMPLE_GAPS) != 0 ? m.q : m.q - 1, plan, state);
    return check_launch(ctx, "annealed importance sampling");
}

// -mJ in ctx->A (ld = n_pad) -> what `t` asks for
static gdca_status score_stage(gdca_ctx *ctx, int N, int sdim, int n_pad, const score_target &t)
{
    hipStream_t s = ctx->stream;
    // the model as the sweep left it, for the fused read-outs: scored on t's sequences in the place of the contact score
    // (a marginal fit of a log-odds run: its sites' range of Pi)
    const gdca_model m{(const double *)ctx->A.p, (size_t)n_pad, -1.0, (const double *)ctx->Pipc.p + (size_t)ctx->pend.site0 * sdim, N, sdim + 1};
    if (t.logodds) return GDCA_OK;  // (the pair stage of a log-odds run needs the joint log det: logodds_epilogue, at collect time)
    switch (t.kind) {
    case score_target::ENERGY:
    case score_target::LOGLIK: return energy_stage(ctx, m, t.X, t.K, t.out, t.strideX);
    case score_target::PAIR: return pair_stage(ctx, m, t.split, t.XA, t.strideA, t.KA, t.XB, t.strideB, t.KB, t.what, t.out);
    case score_target::PARTNER:
        CHK(pair_stage(ctx, m, t.split, t.XA, t.strideA, t.KA, t.XB, t.strideB, t.KB, t.what, t.out, &t.blocks, t.packed));
        return assign_stage(ctx, t.out, t.blocks, t.match, t.gap);
    case score_target::MUTATION: return mutation_stage(ctx, m, t.X, t.K, t.what, t.out);
    case score_target::DOUBLE_SCAN: return double_stage(ctx, m, t.X, t.K, t.out, t.dcode, t.depi, nullptr, 0, nullptr);
    case score_target::DOUBLE_LIST: return double_stage(ctx, m, t.X, t.K, nullptr, nullptr, nullptr, t.muts, t.L, t.out);
    case score_target::WALK: return walk_stage(ctx, m, t.X, t.K, t.walk);
    case score_target::SAMPLE: return sample_stage(ctx, m, t.X, t.K, t.sample);
    case score_target::TEMPER: return temper_stage(ctx, m, t.X, t.K, t.temper);
    case score_target::CONTACT: break;
    }
    double *S_dev = t.out;
    if (t.score == GDCA_SCORE_DI) {
        CHK(ensure(ctx, ctx->Tws, gdca_di_ws_bytes(N, sdim)));
        gdca_launch_di(s, (const double *)ctx->A.p, (size_t)n_pad, (const double *)ctx->Ld.p, N, sdim, S_dev,
                       (double *)ctx->Tws.p, (gdca_dev_scalars *)ctx->sc.p);
    } else {
        CHK(mark(ctx, T_FN_BEGIN));  // (gdca_stats.ms_fn)
        gdca_launch_fn(s, (const double *)ctx->A.p, (size_t)n_pad, N, sdim, S_dev, ctx->ncu);
        CHK(mark(ctx, T_FN_END));
    }
    if (t.apc) {
        CHK(ensure(ctx, ctx->colsum, (size_t)N * sizeof(double)));
        gdca_launch_apc(s, S_dev, N, (double *)ctx->colsum.p);
    }
    return check_launch(ctx, "score");
}

static gdca_status validate(gdca_ctx *ctx, int N, int M, int q)
{
    if (!ctx) return GDCA_EINVAL;
    if (N < 1 || M < 1) return fail(ctx, GDCA_EINVAL, "invalid alignment size");
    if (q < 2 || q > GDCA_MAXQ) return fail(ctx, GDCA_EINVAL, "parameter q is too big (max 31 is allowed)");
    if ((long long)N * (q - 1) > GDCA_MAX_N) return fail(ctx, GDCA_EINVAL, "N*(q-1) is larger than GDCA_MAX_N");
    return GDCA_OK;
}

static gdca_status fetch_scalars(gdca_ctx *ctx)
{
    HIPCHK(hipMemcpyAsync(ctx->sc_host, ctx->sc.p, sizeof(gdca_dev_scalars), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

// An enqueued, not yet collected run (gdca_run_dev_async) owns the ctx workspace: scalars, flags, the pinned item table
// and the big buffers.  Every other entry point that touches the workspace refuses to run until it has been collected.
static gdca_status not_pending(gdca_ctx *ctx)
{
    if (ctx->pending) return fail(ctx, GDCA_EINVAL, "a run is still enqueued on this context: call gdca_run_collect first");
    return GDCA_OK;
}

// The arrays of one host-pointer call, staged on the device: made on the context once the call's arguments have been checked, asked for
// one array at a time, and finished with the status of the `_dev` form.  It does not open on a context with an enqueued run (nothing of
// the context is touched then); the first error sticks, every later request does nothing and yields nullptr, so a caller checks
// status() once.  An absent optional array (host pointer nullptr) stages nothing and yields nullptr.  Each array has a buffer of the
// context's stage_pool to itself, so it starts where hipMalloc put it, and growing the buffer of a later array leaves the earlier
// pointers of the call valid.
// INVARIANT: what is staged for an enqueued run (gdca_run_ranked_async, gdca_run_ranked_phased_async: the alignment gdca_pending::Z
// points at, and the score matrix) stays valid and unchanged until the run's collect -- no host_stage opens on a pending context, and
// nothing else can name the pool's buffers.
class host_stage {
    gdca_ctx *ctx;
    gdca_status st;
    int n = 0;  // arrays staged so far
    struct {
        void *host;
        size_t bytes;
    } back[stage_pool::MAX_ARRAYS];  // where finish() copies array i (host nullptr: nowhere)

    gdca_status hip(hipError_t e) { return e == hipSuccess ? GDCA_OK : fail(ctx, GDCA_EHIP, "staging a host array: %s%s", hipGetErrorString(e), ""); }
    void *stage(const void *from, void *to, size_t bytes)
    {
        if (st == GDCA_OK && n == stage_pool::MAX_ARRAYS) st = fail(ctx, GDCA_EINVAL, "more staged arrays than a call may have");
        if (st != GDCA_OK) return nullptr;
        gdca_buf &b = ctx->staging.buf[n];
        st = ensure(ctx, b, bytes);
        if (st == GDCA_OK && from) st = hip(hipMemcpyAsync(b.p, from, bytes, hipMemcpyHostToDevice, ctx->stream));
        if (st != GDCA_OK) return nullptr;
        back[n].host = to;
        back[n++].bytes = bytes;
        return b.p;
    }

public:
    explicit host_stage(gdca_ctx *c) : ctx(c), st(not_pending(c))
    {
        if (st == GDCA_OK) st = hip(hipSetDevice(c->device));
    }
    gdca_status status() const { return st; }
    // an input, uploaded on the context's stream; an output, which finish() copies to `host` (its size is stated here only); an array
    // the device works on in place, `from` uploaded and the result copied to `to` (the same array, or another); device-only room
    template <class T> const T *in(const T *host, size_t bytes) { return host ? (const T *)stage(host, nullptr, bytes) : nullptr; }
    template <class T> T *out(T *host, size_t bytes) { return host ? (T *)stage(nullptr, host, bytes) : nullptr; }
    template <class T> T *inout(const T *from, T *to, size_t bytes) { return (T *)stage(from, to, bytes); }
    void *room(size_t bytes) { return stage(nullptr, nullptr, bytes); }
    // the first `bytes` of a staged array to the host, enqueued only: finish() waits for it
    void fetch(void *host, const void *dev, size_t bytes)
    {
        if (host && bytes && st == GDCA_OK) st = hip(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    // how a call ends, given the status of its `_dev` form: a failure is returned and nothing copied; otherwise every output comes
    // back (none of zero bytes), with one synchronisation behind the last copy
    gdca_status finish(gdca_status rs)
    {
        if (st != GDCA_OK || rs != GDCA_OK) return st != GDCA_OK ? st : rs;
        for (int i = 0; i < n; ++i) fetch(back[i].host, ctx->staging.buf[i].p, back[i].bytes);
        return st != GDCA_OK ? st : hip(hipStreamSynchronize(ctx->stream));
    }
};

// ||X||_1 of the inverse the sweep has just left in ctx->A (sc->inv_norm1): what the collect decides a refinement on
static gdca_status inverse_norm_stage(gdca_ctx *ctx, int n, int n_pad)
{
    if (ctx->tune.refine == 0) return GDCA_OK;
    CHK(ensure(ctx, ctx->normws, (size_t)n_pad * sizeof(double)));
    gdca_launch_inverse_norm1(ctx->stream, (const double *)ctx->A.p, n_pad, n, (double *)ctx->normws.p,
                              &((gdca_dev_scalars *)ctx->sc.p)->inv_norm1);
    return check_launch(ctx, "inverse_norm1");
}

// ctx->C2 holds the matrix (n_pad x n_pad, identity padding, at least its lower block triangle): dpotrf + dpotri by blocks, -inverse
// into ctx->A where the sweep would have left it; sc->info becomes dpotrf's
static gdca_status cholesky_stage(gdca_ctx *ctx, int n, int n_pad)
{
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    const size_t mat = (size_t)n_pad * n_pad * sizeof(double);
    CHK(ensure(ctx, ctx->B0, mat));
    CHK(ensure(ctx, ctx->Rt, mat));
    CHK(ensure(ctx, ctx->Wd, (size_t)(n_pad / GDCA_TILE) * GDCA_TILE * GDCA_TILE * sizeof(double)));
    HIPCHK(hipMemsetAsync(&sc->info, 0, sizeof(int), ctx->stream));
    gdca_launch_cholesky_inverse(ctx->stream, (double *)ctx->C2.p, (double *)ctx->B0.p, (double *)ctx->Rt.p, (double *)ctx->Wd.p, (double *)ctx->A.p,
                                 n_pad, n, sc, ctx->piv);
    ctx->ld.chol = true;  // (the pivot vector now holds the factor's L_ii^2)
    return check_launch(ctx, "cholesky_inverse");
}

// gdca_run_multi: the covariance of pseudocount pc into dst (ld = n_pad; the padding is the caller's) from the stored Pij_true and the
// kept single-site tallies Pifix -- Pi' of pc (k_pi_finalize), then k_cov_from_pij: bit for bit what tally_stage's mode 1 writes for
// pc.  want_norm1: a group's first build -- sc->pi_max and, where the screen needs it, sc->mat_norm1, as the fused path's first build
// N_all != 0: the principal block of the N sites from site0 on of an alignment of N_all sites, whose Pij_true is the stored one -- Pi' is
// that of all N_all sites (it does not depend on the block), and the block's entries are bit for bit the joint covariance's
static gdca_status cov_from_pij_stage(gdca_ctx *ctx, int N, int M, int q, double pc, double *dst, size_t ld, bool want_norm1, int N_all = 0,
                                      int site0 = 0)
{
    hipStream_t s = ctx->stream;
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    const size_t ldp = (size_t)(N_all ? N_all : N) * (q - 1), off = (size_t)site0 * (q - 1);
    gdca_launch_pi_finalize(s, (const unsigned long long *)ctx->Pifix.p, N_all ? N_all : N, q, gdca_fix_shift(M), &sc->Meff, pc, nullptr,
                            (double *)ctx->Pipc.p, want_norm1 ? &sc->pi_max : nullptr);
    gdca_launch_cov_from_pij(s, (const double *)ctx->Pij.p + off * (ldp + 1), (const double *)ctx->Pipc.p + off, N, q, pc, dst, ld, ldp);
    if (want_norm1 && !gdca_norm1_settled(N, q, pc, ctx->tune.refine, ctx->tune.refine_cond))
        gdca_launch_cov_norm1(s, dst, ld, N, q, pc, ctx->tune.refine_cond, sc, ctx->tune.refine == 1);
    return check_launch(ctx, "covariance from Pij_true");
}

// The covariance of the enqueued run once more into dst (n_pad x n_pad, identity padding), what every rung of the recovery ladder
// starts from (the sweep worked in place): from the tallies -- or, a pseudocount group of gdca_run_multi, from the stored Pij_true
static gdca_status rebuild_padded(gdca_ctx *ctx, void *dst)
{
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    const gdca_pending &r = ctx->pend;
    if (r.pij)
        CHK(cov_from_pij_stage(ctx, r.N, r.M, r.q, r.p.pseudocount, (double *)dst, (size_t)r.n_pad, false, r.N_all, r.site0));
    else
        CHK(tally_stage(ctx, r.Z, r.N, r.M, r.q, &sc->Meff, r.p.pseudocount, 1, nullptr, (double *)dst, (size_t)r.n_pad));
    gdca_launch_pad_identity(ctx->stream, (double *)dst, r.n, r.n_pad);
    return GDCA_OK;
}

// the score stage of the run (pend.target) between its two boundaries; k_fn's are this stage's own
static gdca_status marked_score_stage(gdca_ctx *ctx)
{
    gdca_pending &r = ctx->pend;
    const unsigned fn = 1u << T_FN_BEGIN | 1u << T_FN_END;
    r.ev_marks &= ~fn;
    r.stamp_marks &= ~fn;
    CHK(mark(ctx, T_SCORE_BEGIN));
    CHK(logdet_stage(ctx, r.n));  // (of the inverse the stage reads: a second attempt's and the fallback's come through here again)
    CHK(score_stage(ctx, r.N, r.q - 1, r.n_pad, r.target));
    return mark(ctx, T_END);
}

// ... and ends with: the enqueued run's score stage again on the inverse now in ctx->A, the scalars fetched.  again: the stage of a
// second attempt (or of a further member of a gdca_run_multi group) -- it runs alone and is marked in the run's clock like the first,
// so that ms_score is its time and ms_total ends with it; a refinement or fallback marks k_fn's two again and nothing else (its ms_fn is 0)
static gdca_status rescore(gdca_ctx *ctx, bool again = false)
{
    HIPCHK(hipMemsetAsync(&((gdca_dev_scalars *)ctx->sc.p)->di_noconv, 0, sizeof(int), ctx->stream));
    if (again) ctx->pend.score_batch = 1;
    if (again)
        CHK(marked_score_stage(ctx));
    else {
        CHK(logdet_stage(ctx, ctx->pend.n));
        CHK(score_stage(ctx, ctx->pend.N, ctx->pend.q - 1, ctx->pend.n_pad, ctx->pend.target));
    }
    return fetch_scalars(ctx);
}

static gdca_status begin(gdca_ctx *ctx)
{
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->sc, sizeof(gdca_dev_scalars)));
    gdca_fill_async(ctx->stream, ctx->sc.p, 0, sizeof(gdca_dev_scalars));
    ctx->pend.at = gdca_pending::progress{};
    ctx->pend.timed = false;  // (a fused run opens its timeline next, open_timeline)
    return GDCA_OK;
}

static gdca_status run_inverse(gdca_ctx *ctx);
static gdca_status fill_stats(gdca_ctx *ctx, gdca_stats *st);

// 1/2 (n log 2 pi + log det C), the constant between an energy and a log-likelihood: plain f64, one rounding per operation (one
// multiplication, one addition, one multiplication -- the library is built without contraction), so that a caller who forms it from
// gdca_last_logdet's value the same way gets the same bits
static double loglik_constant(int n, double logdet)
{
    const double a = (double)n * GDCA_LOG_2PI;
    const double b = a + logdet;
    return 0.5 * b;
}

// How a LOGLIK run ends, every collect-time branch behind it: L = -(E + c) in place, c from the log det of the inverse finally used.
// The run's score stage ends with this launch (T_END marked again: ms_score and ms_total include it).
static gdca_status loglik_epilogue(gdca_ctx *ctx)
{
    const score_target &t = ctx->pend.target;
    gdca_launch_loglik(ctx->stream, t.out, t.K, loglik_constant(ctx->pend.n, ctx->ld.val[0]));
    CHK(check_launch(ctx, "loglik"));
    CHK(mark(ctx, T_END));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

// I = -1/2 (log det C - log det C_AA - log det C_BB): plain f64, one rounding per operation (two subtractions, one multiplication), so
// that a caller who forms it from gdca_last_logdet's three values the same way gets the same bits
static double logodds_information(double ld, double ldA, double ldB)
{
    const double a = ld - ldA;
    const double b = a - ldB;
    return -0.5 * b;
}

// How a log-odds run ends, every collect-time branch of the joint fit behind it: the pair stage (full or blocked) on the inverse finally
// used, its gather writing L = ((EmA[a] + EmB[b]) - E[a, b]) + I with I from the three log dets -- the joint one is on the host only
// now --, and for a partner run the assignment on -L.  The run's score stage ends here (T_END marked again); the scalars are fetched
// again: the pair stage's pack has looked at the sequences.
static gdca_status logodds_epilogue(gdca_ctx *ctx)
{
    gdca_pending &r = ctx->pend;
    score_target &t = r.target;
    t.lo.I = logodds_information(ctx->ld.val[0], t.ldA, t.ldB);
    const gdca_model m{(const double *)ctx->A.p, (size_t)r.n_pad, -1.0, (const double *)ctx->Pipc.p, r.N, r.q};
    if (t.kind == score_target::PARTNER) {
        CHK(pair_stage(ctx, m, t.split, t.XA, t.strideA, t.KA, t.XB, t.strideB, t.KB, GDCA_PAIR_ENERGY, t.out, &t.blocks, t.packed, &t.lo));
        CHK(ensure(ctx, ctx->PBN, (size_t)t.blocks.total * sizeof(double)));
        gdca_launch_negate(ctx->stream, t.out, (double *)ctx->PBN.p, (size_t)t.blocks.total);
        CHK(assign_stage(ctx, (const double *)ctx->PBN.p, t.blocks, t.match, t.gap));
    } else {
        CHK(pair_stage(ctx, m, t.split, t.XA, t.strideA, t.KA, t.XB, t.strideB, t.KB, GDCA_PAIR_ENERGY, t.out, nullptr, false, &t.lo));
    }
    CHK(mark(ctx, T_END));
    return fetch_scalars(ctx);
}

// ---- the recovery ladder of an SPD inverse -------------------------------------------------------------------------
// One walk for a fused run's collect and for the operator-level inverses: the decisions are gdca_inverse_outcome.h's, and what differs
// between the two callers is this record and the three functions that read it.
struct inverse_source {
    gdca_inverse_form form;
    const double *A_dev;  // an operator: the caller's matrix (n x n, ld n), still intact -- the sweep works on a copy
};

enum ladder_step { STEP_RETRY, STEP_NEWTON, STEP_FALLBACK };

static gdca_inverse_state ladder_state(const gdca_ctx *ctx, const inverse_source &src, int retries)
{
    const gdca_dev_scalars &h = *ctx->sc_host;
    const gdca_pending &r = ctx->pend;
    const gdca_tuning &t = ctx->tune;
    const bool run = src.form == GDCA_FORM_RUN;  // (an operator has no alignment: no a-priori bound)
    return gdca_inverse_state{src.form, h.info, h.bad_symbol, h.inv_norm1, h.mat_norm1, h.ns_resid, h.pi_max, run ? r.p.pseudocount : 0.0,
                              run ? r.N : 0, run ? r.q : 0, t.refine, t.cholesky, t.refine_cond, r.at.attempt, retries};
}

// the matrix once more into dst (n_pad x n_pad, identity padding): a run's covariance from the tallies or the stored Pij_true, an
// operator's from the caller
static gdca_status ladder_matrix(gdca_ctx *ctx, const inverse_source &src, void *dst)
{
    if (src.form == GDCA_FORM_RUN) return rebuild_padded(ctx, dst);
    gdca_launch_copy_in(ctx->stream, src.A_dev, ctx->pend.n, (double *)dst, ctx->pend.n_pad);
    return check_launch(ctx, "copy_in");
}

// ||X||_1 of the inverse in ctx->A into sc->inv_norm1; an operator measures ||C||_1 of the caller's matrix with it (a run's first
// build of the covariance has done that where the screen needed it)
static gdca_status ladder_norms(gdca_ctx *ctx, const inverse_source &src)
{
    if (src.form == GDCA_FORM_OPERATOR) {
        CHK(ensure(ctx, ctx->normws, (size_t)ctx->pend.n_pad * sizeof(double)));
        gdca_launch_matrix_norm1(ctx->stream, src.A_dev, (size_t)ctx->pend.n, ctx->pend.n, (double *)ctx->normws.p,
                                 &((gdca_dev_scalars *)ctx->sc.p)->mat_norm1);
    }
    return inverse_norm_stage(ctx, ctx->pend.n, ctx->pend.n_pad);
}

// what follows an inverse that changed; the scalars are in sc_host afterwards.  A run scores again -- a second attempt as a stage of
// its own on the run's timeline, and after the fallback gdca_stats.inverse_norm1 is that inverse's.  An operator takes the log det of
// the new pivots; after a Newton-Schulz step its log det stays that of the sweep's pivots.
static gdca_status ladder_changed(gdca_ctx *ctx, const inverse_source &src, ladder_step step)
{
    if (src.form == GDCA_FORM_OPERATOR) {
        if (step != STEP_NEWTON) CHK(logdet_stage(ctx, ctx->pend.n));
        return fetch_scalars(ctx);
    }
    if (step == STEP_FALLBACK) CHK(inverse_norm_stage(ctx, ctx->pend.n, ctx->pend.n_pad));
    CHK(rescore(ctx, step == STEP_RETRY));
    if (step == STEP_RETRY) ctx->pend.at.rescored = true;
    return GDCA_OK;
}

// A first attempt has completed and its scalars are in sc_host: up to `retries` further attempts where the watchdog ended the launch,
// the norm, the Newton-Schulz step and the Cholesky fallback, each where gdca_inverse_outcome.h says so -- on ordinary input every
// answer is no and nothing is enqueued.  Synchronous and several times the cost of the inverse itself wherever a rung is taken: the
// paths of rare inputs (pseudocounts far below the 0.2 .. 0.8 gDCA is used with), walked here so that the enqueue side stays lean.
// The inverse finally arrived at is in ctx->A, its scalars in sc_host, what was done to it in pend.at.
static gdca_status inverse_ladder(gdca_ctx *ctx, const inverse_source &src, int retries)
{
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    const int n = ctx->pend.n, n_pad = ctx->pend.n_pad;
    const size_t mat = (size_t)n_pad * n_pad * sizeof(double);
    while (gdca_retry_due(ladder_state(ctx, src, retries))) {
        // (a run's inverse again as a launch of its own behind the pipeline's gate, marked on the run's timeline)
        ++ctx->pend.at.attempt;
        CHK(ladder_matrix(ctx, src, ctx->A.p));
        HIPCHK(hipMemsetAsync(&sc->info, 0, sizeof(int), ctx->stream));
        CHK(src.form == GDCA_FORM_RUN ? run_inverse(ctx) : inverse_stage(ctx, n, n_pad, nullptr));
        CHK(ladder_changed(ctx, src, STEP_RETRY));
    }
    if (gdca_norm_due(ladder_state(ctx, src, retries))) {
        CHK(ladder_norms(ctx, src));
        CHK(fetch_scalars(ctx));
    }
    if (gdca_wants_refinement(ladder_state(ctx, src, retries))) {
        CHK(ensure(ctx, ctx->C2, mat));
        CHK(ensure(ctx, ctx->B0, mat));
        CHK(ensure(ctx, ctx->Rt, mat));
        CHK(ladder_matrix(ctx, src, ctx->C2.p));
        gdca_launch_newton_schulz(ctx->stream, (double *)ctx->A.p, (const double *)ctx->C2.p, (double *)ctx->B0.p, (double *)ctx->Rt.p, n_pad,
                                  &sc->ns_resid);
        CHK(check_launch(ctx, "newton_schulz"));
        CHK(ladder_changed(ctx, src, STEP_NEWTON));
        ctx->pend.at.refined = gdca_refined_after_step(ladder_state(ctx, src, retries));
    }
    if (gdca_wants_cholesky(ladder_state(ctx, src, retries), ctx->pend.at.refined)) {
        // blocked dpotrf + dpotri of the matrix: its verdict on positive definiteness is LAPACK's
        CHK(ensure(ctx, ctx->C2, mat));
        CHK(ladder_matrix(ctx, src, ctx->C2.p));
        CHK(cholesky_stage(ctx, n, n_pad));
        CHK(ladder_changed(ctx, src, STEP_FALLBACK));
        ctx->pend.at.refined = 2;
    }
    return GDCA_OK;
}

extern "C" {

gdca_status gdca_run_collect(gdca_ctx *ctx, gdca_stats *st)
{
    if (!ctx) return GDCA_EINVAL;
    if (!ctx->pending) return fail(ctx, GDCA_EINVAL, "no enqueued run to collect");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->pending = false;
    ctx->pend.rank.pending = false;  // (collected through this entry, a ranked run's ranking is given up: its arrays are scratch of the next run)
    if (ctx->pend.sc_published) {
        // the run's last kernel wrote the scalars to sc_host: no copy of the runtime's -- a kernel -- behind another context's sweep
        ctx->pend.sc_published = false;
        HIPCHK(hipStreamSynchronize(ctx->stream));
    } else {
        CHK(fetch_scalars(ctx));
    }
    CHK(inverse_ladder(ctx, inverse_source{GDCA_FORM_RUN, nullptr}, ctx->tune.sweep_retries));
    note_logdet(ctx);
    if (ctx->pend.target.kind == score_target::LOGLIK && ctx->sc_host->info == 0 && !ctx->sc_host->bad_symbol) CHK(loglik_epilogue(ctx));
    if (ctx->pend.target.logodds && ctx->sc_host->info == 0 && !ctx->sc_host->bad_symbol) CHK(logodds_epilogue(ctx));
    if (st) CHK(fill_stats(ctx, st));
    const gdca_status verdict = conclude(ctx, GDCA_ENDS_RUN);
    if (verdict == GDCA_ENOCONV && st) st->info = -ctx->sc_host->di_noconv;
    return verdict;
}

}  // extern "C"

// the times that end with the score stage just run: of the collected run, or of a further member of a gdca_run_multi group
static gdca_status score_times(gdca_ctx *ctx, gdca_stats *st)
{
    bool tfail = false;
    const double sbatch = (double)(ctx->pend.score_batch > 0 ? ctx->pend.score_batch : 1);
    st->ms_total = elapsed(ctx, T_BEGIN, T_END, &tfail);
    st->ms_score = elapsed(ctx, T_SCORE_BEGIN, T_END, &tfail) / sbatch;
    st->ms_fn = ctx->pend.at.refined == 0 ? elapsed(ctx, T_FN_BEGIN, T_FN_END, &tfail) / sbatch : 0.0;
    if (tfail) return fail(ctx, GDCA_EHIP, "hipEventElapsedTime");
    return GDCA_OK;
}

// gdca_stats of the run just collected: the scalars in sc_host, the pending record and its stage times (all 0 for an untimed run)
static gdca_status fill_stats(gdca_ctx *ctx, gdca_stats *st)
{
    const gdca_dev_scalars &h = *ctx->sc_host;
    memset(st, 0, sizeof(*st));
    st->theta = h.theta;
    st->Meff = h.Meff;
    st->pair_identity_sum = h.pair_sum;
    st->thresh = h.thresh;
    st->info = h.info;
    st->N = ctx->pend.N;
    st->M = ctx->pend.M;
    st->q = ctx->pend.q;
    st->n = ctx->pend.n;
    st->n_pad = ctx->pend.n_pad;
    st->update_launches = ctx->pend.n_upd;
    st->inverse_batch = ctx->pend.batch;
    st->refined = ctx->pend.at.refined;
    st->sweep_retries = ctx->pend.at.attempt;
    st->inverse_norm1 = h.inv_norm1;
    st->matrix_norm1 = h.mat_norm1;
    st->cond_bound = ctx->tune.refine != 0 ? gdca_cond_bound(h.mat_norm1, h.pi_max, ctx->pend.p.pseudocount, ctx->pend.q, ctx->pend.N) : 0.0;
    st->inverse_flops = inverse_flops_model((double)ctx->pend.n);
    st->update_flops = ctx->pend.upd_flops;
    st->sweep_ghz = h.sweep_ticks ? (double)h.sweep_cycles / (double)h.sweep_ticks * 0.1 : 0.0;
    bool tfail = false;
    // (stages issued as batched grids carry the whole batch: a member reports its share, as for a merged inverse -- a family whose
    // inverse shared a merged launch with others reports the launch's time divided by the families it carried: the sum over the
    // members is the launch)
    const double fshare = 1.0 / (double)(ctx->pend.front_batch > 0 ? ctx->pend.front_batch : 1);
    const double share = 1.0 / (double)(ctx->pend.batch > 0 ? ctx->pend.batch : 1);
    st->ms_theta = elapsed(ctx, T_BEGIN, T_THETA, &tfail) * fshare;
    st->ms_weights = elapsed(ctx, T_THETA, T_WEIGHTS, &tfail) * fshare;
    st->ms_covariance = elapsed(ctx, T_WEIGHTS, T_COV, &tfail) * fshare;
    if (ctx->pend.at.refined == 0) st->ms_pair_tally = elapsed(ctx, T_TALLY_BEGIN, T_TALLY_END, &tfail) * fshare;
    st->ms_inverse = elapsed(ctx, T_INV_BEGIN, T_INV_END, &tfail) * share;
    st->ms_inverse_update = elapsed(ctx, T_SWEEP_BEGIN, T_SWEEP_END, &tfail) * share;
    if (tfail) return fail(ctx, GDCA_EHIP, "hipEventElapsedTime");
    return score_times(ctx, st);
}

// The three phases of one run, enqueued on `s` (the ctx's own stream, or the leader's when several families are batched by
// phase): front end (theta, reweighting, tallies, covariance), SPD inverse, scores.
static gdca_status check_params(gdca_ctx *ctx, const gdca_params *p)
{
    if (!(p->pseudocount >= 0.0 && p->pseudocount <= 1.0)) return fail(ctx, GDCA_EINVAL, "invalid pseudocount value (must be between 0 and 1)");
    if (!(p->theta <= 1.0)) return fail(ctx, GDCA_EINVAL, "invalid theta value");
    return GDCA_OK;
}

static gdca_status run_check_args(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                  double *S_dev)
{
    CHK(validate(ctx, N, M, q));
    if (!Z_dev || !S_dev || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(check_params(ctx, p));
    if (p->score != GDCA_SCORE_FROB && p->score != GDCA_SCORE_DI) return fail(ctx, GDCA_EINVAL, "invalid score value");
    return GDCA_OK;
}

// the front-end part of the pending record.  pij: the stored Pij_true of gdca_run_multi, nullptr for a single run
static void pending_front(gdca_ctx *ctx, const int8_t *Z_dev, int N, int M, int q, const gdca_params *p, const double *pij)
{
    gdca_pending &r = ctx->pend;
    r.N = N;
    r.M = M;
    r.q = q;
    r.n = N * (q - 1);
    r.n_pad = round_up(r.n, GDCA_TILE);
    r.Z = Z_dev;
    r.pij = pij;
    r.N_all = r.site0 = 0;  // (run_logodds knows better)
    r.p = *p;
    r.front_batch = r.score_batch = 1;  // (run_phased knows better)
}

// how every fused run opens: its timeline (stamped: a member of a batch issued as batched grids), theta and the reweighting
static gdca_status front_weights(gdca_ctx *ctx, const int8_t *Z_dev, int N, int M, int q, double theta, bool stamped)
{
    CHK(begin(ctx));  // (one run may be outstanding per ctx: its scalars and events would be overwritten -> GDCA_EINVAL)
    CHK(open_timeline(ctx, ctx->timing, stamped));
    CHK(mark(ctx, T_BEGIN));
    CHK(weights_stage(ctx, Z_dev, N, M, q, theta, -1, false));
    return mark(ctx, T_WEIGHTS);
}

// ... and how the covariance in ctx->A (ld = n_pad) becomes the inverse's input: its identity padding, and for the DI score its
// diagonal blocks saved and factored
static gdca_status covariance_tail(gdca_ctx *ctx, int N, int sdim, int n_pad, bool di)
{
    hipStream_t s = ctx->stream;
    gdca_launch_pad_identity(s, (double *)ctx->A.p, N * sdim, n_pad);
    if (di) {
        CHK(ensure(ctx, ctx->Dblk, (size_t)N * sdim * sdim * sizeof(double)));
        CHK(ensure(ctx, ctx->Ld, (size_t)N * sdim * sdim * sizeof(double)));
        gdca_launch_save_diag_blocks(s, (const double *)ctx->A.p, (size_t)n_pad, N, sdim, (double *)ctx->Dblk.p);
        gdca_launch_diag_chol(s, (const double *)ctx->Dblk.p, N, sdim, (double *)ctx->Ld.p);
    }
    CHK(check_launch(ctx, "covariance"));
    return mark(ctx, T_COV);
}

static gdca_status run_front(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, bool stamped = false)
{
    CHK(front_weights(ctx, Z_dev, N, M, q, p->theta, stamped));
    const int sdim = q - 1, n_pad = round_up(N * sdim, GDCA_TILE);
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    CHK(ensure(ctx, ctx->A, (size_t)n_pad * n_pad * sizeof(double)));
    CHK(tally_stage(ctx, Z_dev, N, M, q, &sc->Meff, p->pseudocount, 1, nullptr, (double *)ctx->A.p, (size_t)n_pad, ctx->tune.refine != 0));
    CHK(covariance_tail(ctx, N, sdim, n_pad, p->score == GDCA_SCORE_DI));
    pending_front(ctx, Z_dev, N, M, q, p, nullptr);
    return GDCA_OK;
}

// the inverse of the context's run as a launch of its own: bracketed by events, inside a stamped run too
static gdca_status run_inverse(gdca_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    double upd_flops = 0.0;
    if (ctx->gate) HIPCHK(gate_wait(ctx->gate, s));
    CHK(mark(ctx, T_INV_BEGIN, true));  // start of this family's turn on the MFMA pipe
    CHK(inverse_stage(ctx, ctx->pend.n, ctx->pend.n_pad, &upd_flops));
    CHK(mark(ctx, T_INV_END, true));
    if (ctx->gate) HIPCHK(gate_pass(ctx->gate, s));
    ctx->pend.n_upd = 1;
    ctx->pend.upd_flops = upd_flops;
    ctx->pend.batch = 1;
    return GDCA_OK;
}

// The inverses of K members of a phase batch as ONE merged launch on the batch's stream (k_sweep_merged: small matrices, which
// leave most of the chip idle when they run alone).  Every member keeps its own workspace, flags, scalars and events.
static gdca_status run_inverse_merged(gdca_ctx *lead, gdca_ctx *const *mem, int K)
{
    gdca_ctx *ctx = mem[0];
    hipStream_t s = ctx->stream;
    gdca_inverse_job jobs[8];
    gdca_tuning tun[8];  // a member's schedule switches are its own context's, the switches of the merged launch the leader's
    double flops[8];
    if (K > gdca_inverse_max_merge() || K > 8) return fail(ctx, GDCA_EINVAL, "too many members in a merged inverse");
    bool timed = true, stamps = true;
    // (the members of a batch are normally peers of ONE pipeline: one wait and one record per distinct gate, not per member)
    gdca_gate *gates[8];
    int n_gates = 0;
    for (int k = 0; k < K; ++k) {
        timed = timed && mem[k]->pend.timed;
        stamps = stamps && mem[k]->pend.stamped;
        gdca_gate *g = mem[k]->gate;
        bool seen = !g;
        for (int j = 0; j < n_gates && !seen; ++j) seen = gates[j] == g;
        if (!seen) {
            gates[n_gates++] = g;
            HIPCHK(gate_wait(g, s));
        }
    }
    for (int k = 0; k < K; ++k) {
        mem[k]->pend.timed = timed;  // (the launch is timed for all its members or for none)
        CHK(inverse_job(mem[k], mem[k]->pend.n, mem[k]->pend.n_pad, &jobs[k]));
        tun[k] = mem[k]->tune;
        tun[k].merge_group = lead->tune.merge_group;
        tun[k].merge_mcus = lead->tune.merge_mcus;
        jobs[k].tune = &tun[k];
        if (lead->tune.sweep_debug & 16) CHK(poison_inverse_ws(mem[k], s));
    }
    if (timed) CHK(mark_members(s, mem, K, T_INV_BEGIN, T_SWEEP_BEGIN, stamps));
    gdca_launch_spd_inverse_merged(s, jobs, K, nullptr, nullptr, flops);
    CHK(check_launch(ctx, "spd_inverse_merged"));
    if (timed) CHK(mark_members(s, mem, K, T_SWEEP_END, T_INV_END, stamps));
    for (int j = 0; j < n_gates; ++j) HIPCHK(gate_pass(gates[j], s));
    for (int k = 0; k < K; ++k) {
        mem[k]->pend.n_upd = k == 0 ? 1 : 0;
        mem[k]->pend.upd_flops = flops[k];
        mem[k]->pend.batch = K;
    }
    return GDCA_OK;
}

static gdca_status run_score(gdca_ctx *ctx, const score_target &t)
{
    ctx->pend.target = t;
    // (the start of THIS run's score stage: in a phase batch the members' stages follow one another behind the shared inverse)
    CHK(marked_score_stage(ctx));
    ctx->pend.sc_published = false;
    if (ctx->sc_host_dev) {
        gdca_launch_publish_scalars(ctx->stream, (const gdca_dev_scalars *)ctx->sc.p, ctx->sc_host_dev);
        CHK(check_launch(ctx, "publish_scalars"));
        ctx->pend.sc_published = true;
    }
    ctx->pending = true;
    return GDCA_OK;
}

// The inverses of the members of a batch, all enqueued on the batch's stream (every member's `stream` points there, pend.n /
// pend.n_pad are set): those of the small members (up to `merge_blocks` 128-blocks: chain-bound single-block schedules that leave
// most of the chip idle) are carried `merge` at a time by ONE launch (options GDCA_MERGE, GDCA_MERGE_BLOCKS of the leader; bit for
// bit the results of launches of their own), the others run back to back
static gdca_status run_inverses(gdca_ctx *lead, gdca_ctx *const *ctxs, int K)
{
    gdca_ctx *small[64];
    int n_small = 0;
    gdca_status st = GDCA_OK;
    const int merge = std::min(lead->tune.merge, gdca_inverse_max_merge());
    for (int k = 0; k < K && st == GDCA_OK; ++k) {
        if (merge > 1 && ctxs[k]->pend.n_pad / GDCA_TILE <= lead->tune.merge_blocks)
            small[n_small++] = ctxs[k];
        else
            st = run_inverse(ctxs[k]);
    }
    // A launch is closed when it holds `merge` members or its members together offer MERGE_TILES tile items per update step
    // (sum of nblk^2 / 2: enough work beside a member's chain -- ~250 us per group of four blocks against ~0.2 us per tile item
    // on the whole chip; 20-block matrices go eight to a launch, 47-block ones two).  A lone last member joins the launch
    // before it.
    int start[65], n_grp = 0;
    {
        long long tiles = 0;
        int cnt = 0;
        for (int k = 0; k < n_small; ++k) {
            if (cnt == 0) start[n_grp++] = k;
            const long long nb = small[k]->pend.n_pad / GDCA_TILE;
            tiles += nb * nb / 2;
            ++cnt;
            if (cnt == merge || tiles >= lead->tune.merge_tiles) {
                cnt = 0;
                tiles = 0;
            }
        }
        start[n_grp] = n_small;
        if (n_grp >= 2 && start[n_grp] - start[n_grp - 1] == 1 && start[n_grp - 1] - start[n_grp - 2] < merge) start[--n_grp] = n_small;
    }
    for (int gi = 0; gi < n_grp && st == GDCA_OK; ++gi) {
        const int at = start[gi], cnt = start[gi + 1] - at;
        // (option SWEEP_DEBUG bit 3, tests: the merged kernel for a single member too)
        st = (cnt == 1 && !(lead->tune.sweep_debug & 8)) ? run_inverse(small[at]) : run_inverse_merged(lead, small + at, cnt);
    }
    return st;
}

extern "C" {

gdca_status gdca_run_dev_async(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q,
                               const gdca_params *p, double *S_dev)
{
    CHK(run_check_args(ctx, Z_dev, N, M, q, p, S_dev));
    CHK(run_front(ctx, Z_dev, N, M, q, p));
    CHK(run_inverse(ctx));
    return run_score(ctx, contact_target(p->score, p->apc, S_dev));
}

static gdca_status ranking_stage(gdca_ctx *ctx, const double *S_dev, int N, int sep, long long len, int32_t **ii, int32_t **jj, double **sc);

// the ranking of an enqueued run behind its scores, before anybody waits: one synchronisation for the whole run
static void enqueue_ranking(gdca_ctx *ctx, const double *S_dev, int N, int sep)
{
    auto &r = ctx->pend.rank;
    r.len = gdca_ranking_length(N, sep);
    r.sep = sep;
    r.status = r.len > 0 ? ranking_stage(ctx, S_dev, N, sep, r.len, &r.i, &r.j, &r.s) : GDCA_OK;
    r.pending = true;
}

static gdca_status run_phased(gdca_ctx *const *ctxs, int32_t K, const int8_t *const *Z_dev, const int32_t *N, const int32_t *M, const int32_t *q,
                              const gdca_params *p, double *const *S_dev, int rank_sep, bool *ranked)
{
    if (ranked) *ranked = false;
    if (!ctxs || K < 1 || !Z_dev || !N || !M || !q || !p || !S_dev) return GDCA_EINVAL;
    gdca_ctx *lead = ctxs[0];
    if (!lead) return GDCA_EINVAL;
    for (int k = 0; k < K; ++k) {
        if (!ctxs[k]) return fail(lead, GDCA_EINVAL, "null context in the batch");
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return fail(lead, GDCA_EINVAL, "the same context twice in one batch");
        if (ctxs[k]->device != lead->device) return fail(lead, GDCA_EINVAL, "contexts of one batch must share a device");
        gdca_status vs = not_pending(ctxs[k]);
        if (vs == GDCA_OK) vs = run_check_args(ctxs[k], Z_dev[k], N[k], M[k], q[k], p, S_dev[k]);
        if (vs != GDCA_OK) return member_error(lead, ctxs[k], k, vs);
    }
    // Phase by phase: K front ends, K inverses back to back, K score stages.  The inverses and the score stages go to the leader's
    // stream.  The front ends (reweighting, tallies, covariance: kernels of a few dozen to a few hundred workgroups each for a small
    // family -- the pair tally of an N = 128 family launches 36 on 256 compute units) run SIDE BY SIDE, each on its member's own
    // stream, and the leader's stream waits for all of them before the first inverse (option PHASED_FRONTS=0: one after the other
    // on the leader's stream, as in round 4: 8 x 0.55 ms in front of 8 x 0.43 ms of merged inverses at config B).  The members keep
    // their own workspaces, scalars and timing events; their streams are restored before returning.
    hipStream_t own[64], use[64];
    if (K > 64) return fail(lead, GDCA_EINVAL, "at most 64 families per batch");
    // Round 6, the default (option PHASED_GRIDS != 0): the members' kernels of a KIND as ONE grid (gdca_launch.h).  The front ends are
    // recorded member by member, then issued in lockstep on the leader's stream -- ~25 launches per batch instead of ~25 per member,
    // every one with all members' workgroups on the chip at once --, then the inverses, then the score stages (and, for the ranked
    // entry, the rankings) the same way.  Stage boundaries are time stamps written by kernels of the batch, not events.  Bit for bit
    // the results of the other schedules: a kernel body cannot tell which launch form runs it.
    if (lead->tune.phased_grids != 0 && K > 1) {  // (-1: the rule below; 1 .. 8: that many groups)
        for (int k = 0; k < K; ++k) {
            own[k] = ctxs[k]->stream;
            if (k > 0) (void)hipStreamSynchronize(own[k]);  // nothing of an earlier use is still in flight on the member's own stream
        }
        gdca_status st = GDCA_OK;
        int done_front = 0, failed = -1;
        gdca_recorder rec;
        // the batch's stream: the pipeline's (gdca_gate) where the leader belongs to one, behind whatever its own stream holds
        hipStream_t bs = lead->gate && lead->gate->batch_stream ? lead->gate->batch_stream : lead->stream;
        if (bs != lead->stream && (hipEventRecord(lead->ev_upload, lead->stream) != hipSuccess || hipStreamWaitEvent(bs, lead->ev_upload, 0) != hipSuccess))
            return fail(lead, GDCA_EHIP, "event chain of the batch");
        // G groups of members (member k in group k mod G), each group's front ends as batched grids on a stream of its own -- the
        // leader's and the next members' --, the groups side by side: a VALU-bound reweighting of one group runs beside the
        // LDS-atomic-bound pair tallies of another.  One group (everything in lockstep) where the members are small: their kernels
        // are launch-bound and two groups would be twice the launches.
        int G = lead->tune.phased_grids;
        if (G < 0) {
            double work = 0.0;  // symbol compares + tallies of the batch's front ends
            for (int k = 0; k < K; ++k) work += 0.5 * (double)M[k] * (double)M[k] * (double)N[k] + 0.5 * (double)N[k] * (double)N[k] * (double)M[k];
            G = work / K > 2e10 ? 4 : 1;
        }
        G = std::max(1, std::min(std::min(G, (int)K), 8));
        int in_group[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int gi = 0; gi < G && st == GDCA_OK; ++gi) {
            hipStream_t sg = gi == 0 ? bs : own[gi];
            rec.begin(sg, K);
            for (int k = gi; k < K && st == GDCA_OK; k += G) {
                ctxs[k]->stream = sg;
                rec.member(k);
                st = run_front(ctxs[k], Z_dev[k], N[k], M[k], q[k], p, true);
                if (st == GDCA_OK) {
                    ++done_front;
                    ++in_group[gi];
                } else {
                    failed = k;
                }
            }
            rec.member(-1);
            if (rec.flush() != hipSuccess && st == GDCA_OK) st = fail(lead, GDCA_EHIP, "a batched front-end launch failed");
            // the batch's stream goes on behind this group's front ends
            if (st == GDCA_OK && gi > 0 &&
                (hipEventRecord(ctxs[gi]->ev_batch, sg) != hipSuccess || hipStreamWaitEvent(bs, ctxs[gi]->ev_batch, 0) != hipSuccess))
                st = fail(lead, GDCA_EHIP, "event chain of the batch's front ends");
        }
        if (st != GDCA_OK) done_front = 0;  // (nothing of a batch that failed to enqueue is run any further; it is drained below)
        for (int k = 0; k < K; ++k) {
            ctxs[k]->stream = bs;
            if (st == GDCA_OK) ctxs[k]->pend.front_batch = in_group[k % G];
        }
        rec.begin(bs, K);
        if (st == GDCA_OK) st = run_inverses(lead, ctxs, done_front);
        for (int k = 0; k < done_front && st == GDCA_OK; ++k) {
            rec.member(k);
            ctxs[k]->pend.score_batch = done_front;
            st = run_score(ctxs[k], contact_target(p->score, p->apc, S_dev[k]));
            if (st == GDCA_OK && rank_sep > 0) enqueue_ranking(ctxs[k], S_dev[k], N[k], rank_sep);
            if (st != GDCA_OK) failed = k;
        }
        rec.member(-1);
        if (rec.end() != hipSuccess && st == GDCA_OK) st = fail(lead, GDCA_EHIP, "a batched score launch failed");
        if (ranked && st == GDCA_OK && rank_sep > 0) *ranked = true;
        // the members' collects synchronise THEIR stream: every one of them waits for the batch (one event on the batch's stream)
        bool chained = st == GDCA_OK && hipEventRecord(lead->ev_batch, bs) == hipSuccess;
        for (int k = bs == own[0] ? 1 : 0; k < K && chained; ++k) chained = hipStreamWaitEvent(own[k], lead->ev_batch, 0) == hipSuccess;
        for (int k = 0; k < K; ++k) ctxs[k]->stream = own[k];
        if (st != GDCA_OK) {
            (void)hipStreamSynchronize(bs);
            for (int k = 0; k < K; ++k) {
                (void)hipStreamSynchronize(own[k]);  // (a group's front ends)
                ctxs[k]->pending = false;
                ctxs[k]->pend.rank.pending = false;
            }
            return failed > 0 ? member_error(lead, ctxs[failed], failed, st) : st;
        }
        if (!chained) {
            (void)hipStreamSynchronize(bs);
            return fail(lead, GDCA_EHIP, "event chain of the batch");
        }
        return GDCA_OK;
    }
    const bool side_by_side = lead->tune.phased_fronts != 0 && K > 1;
    // ... on the streams of the first PHASED_STREAMS members, round robin (default 4, the runtime's hardware queues: with one
    // stream per member the eight front ends of a config-B batch ran two to three wide and started up to 1.4 ms apart,
    // profiles/r05_B_merged8_timeline.log -- streams that share a hardware queue take turns, and the second of a pair started
    // hundreds of microseconds after the first had finished)
    const int W = side_by_side ? std::max(1, std::min((int)K, lead->tune.phased_streams)) : 1;
    for (int k = 0; k < K; ++k) {
        own[k] = ctxs[k]->stream;
        if (k > 0) (void)hipStreamSynchronize(own[k]);  // nothing of an earlier use is still in flight on the member's own stream
    }
    for (int k = 0; k < K; ++k) use[k] = side_by_side ? own[k % W] : lead->stream;
    gdca_status st = GDCA_OK;
    int done_front = 0;
    for (int k = 0; k < K && st == GDCA_OK; ++k) {
        ctxs[k]->stream = use[k];
        st = run_front(ctxs[k], Z_dev[k], N[k], M[k], q[k], p);
        if (st == GDCA_OK && use[k] != lead->stream) {
            // the batch's stream goes on behind this member's front end
            if (hipEventRecord(ctxs[k]->ev_batch, use[k]) != hipSuccess || hipStreamWaitEvent(lead->stream, ctxs[k]->ev_batch, 0) != hipSuccess)
                st = fail(lead, GDCA_EHIP, "event chain of the batch's front ends");
        }
        if (st == GDCA_OK) ++done_front;
    }
    for (int k = 0; k < K; ++k) ctxs[k]->stream = lead->stream;
    if (st == GDCA_OK) st = run_inverses(lead, ctxs, done_front);
    if (st == GDCA_OK && side_by_side) {
        // ... and the score stages side by side again, each behind the batch's inverses on the stream its front end ran on
        if (hipEventRecord(lead->ev_upload, lead->stream) != hipSuccess) st = fail(lead, GDCA_EHIP, "event chain of the batch's score stages");
        for (int j = 1; j < W && st == GDCA_OK; ++j)
            if (hipStreamWaitEvent(own[j], lead->ev_upload, 0) != hipSuccess) st = fail(lead, GDCA_EHIP, "event chain of the batch's score stages");
    }
    bool chained = true;  // every member's own stream waits for what was enqueued for it elsewhere
    for (int k = 0; k < done_front && st == GDCA_OK; ++k) {
        ctxs[k]->stream = use[k];
        st = run_score(ctxs[k], contact_target(p->score, p->apc, S_dev[k]));
        // the members' collects synchronise THEIR stream: make it wait for the stream the member's work went to (one event per member)
        if (st == GDCA_OK && use[k] != own[k] &&
            (hipEventRecord(ctxs[k]->ev_batch, use[k]) != hipSuccess || hipStreamWaitEvent(own[k], ctxs[k]->ev_batch, 0) != hipSuccess))
            chained = false;
    }
    if (st != GDCA_OK) {
        // a member failed to enqueue (allocation, launch): drain what was enqueued -- the batch's stream AND every member's own
        // stream -- and leave nobody half-pending.  The failing member's message goes to the leader, whose last_error the caller reads.
        (void)hipStreamSynchronize(lead->stream);
        for (int k = 0; k < K; ++k) {
            (void)hipStreamSynchronize(own[k]);  // (a front end enqueued side by side)
            ctxs[k]->pending = false;
            if (k == done_front) member_error(lead, ctxs[k], k, st);
        }
    }
    for (int k = 0; k < K; ++k) ctxs[k]->stream = own[k];
    if (st == GDCA_OK && !chained) {
        // the chain could not be built: the members' collects would not wait for the batch -- wait for it here instead
        (void)hipStreamSynchronize(lead->stream);
        for (int j = 1; j < W; ++j) (void)hipStreamSynchronize(own[j]);
        return fail(lead, GDCA_EHIP, "event chain of the batch");
    }
    return st;
}

gdca_status gdca_run_dev_phased(gdca_ctx *const *ctxs, int32_t K, const int8_t *const *Z_dev, const int32_t *N,
                                const int32_t *M, const int32_t *q, const gdca_params *p, double *const *S_dev)
{
    return run_phased(ctxs, K, Z_dev, N, M, q, p, S_dev, 0, nullptr);
}

gdca_status gdca_run_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                         double *S_dev, gdca_stats *st)
{
    CHK(gdca_run_dev_async(ctx, Z_dev, N, M, q, p, S_dev));
    return gdca_run_collect(ctx, st);
}

gdca_status gdca_run(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                     double *S_host, gdca_stats *st)
{
    CHK(validate(ctx, N, M, q));
    if (!Z_host || !S_host) return fail(ctx, GDCA_EINVAL, "null pointer");
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    double *S_dev = sg.out(S_host, (size_t)N * N * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_dev(ctx, Z_dev, N, M, q, p, S_dev, st));
}

// ---- compute_ranking on the device (src/GaussDCA.jl:88-99, call :44) ---------------------------------------
static gdca_status ranking_stage(gdca_ctx *ctx, const double *S_dev, int N, int sep, long long len, int32_t **ii, int32_t **jj, double **sc)
{
    CHK(ensure(ctx, ctx->rankws, gdca_ranking_ws_bytes(len)));
    gdca_launch_ranking(ctx->stream, S_dev, N, sep, len, ctx->rankws.p, ii, jj, sc);
    return check_launch(ctx, "ranking");
}

static gdca_status ranking_to_host(gdca_ctx *ctx, long long len, const int32_t *ii, const int32_t *jj, const double *sc, int32_t *i_out, int32_t *j_out,
                                   double *score_out)
{
    HIPCHK(hipMemcpyAsync(i_out, ii, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(j_out, jj, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(score_out, sc, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

gdca_status gdca_ranking_dev(gdca_ctx *ctx, const double *S_dev, int32_t N, int32_t min_separation, int32_t *i_out, int32_t *j_out, double *score_out)
{
    if (!ctx || !S_dev || N < 1 || N > 65535 || min_separation < 1) return GDCA_EINVAL;
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    const long long len = gdca_ranking_length(N, min_separation);
    if (len == 0) return GDCA_OK;
    if (!i_out || !j_out || !score_out) return GDCA_EINVAL;
    int32_t *ii, *jj;
    double *sc;
    CHK(ranking_stage(ctx, S_dev, N, min_separation, len, &ii, &jj, &sc));
    return ranking_to_host(ctx, len, ii, jj, sc, i_out, j_out, score_out);
}

gdca_status gdca_run_ranked_async(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t min_separation)
{
    CHK(validate(ctx, N, M, q));
    if (!Z_host || min_separation < 1) return fail(ctx, GDCA_EINVAL, "null pointer or min_separation < 1");
    // (from pageable memory this copy holds the calling thread until the last byte is staged -- and overlaps whatever another
    // context of the same device is computing meanwhile: the pipelined batch driver's upload of the NEXT family)
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    double *S_dev = (double *)sg.room((size_t)N * N * sizeof(double));  // (both stay the run's until its collect: host_stage)
    CHK(sg.status());
    CHK(upload_done(ctx));  // Z_host is the caller's again when this call returns (gdca.h), pinned or not
    CHK(gdca_run_dev_async(ctx, Z_dev, N, M, q, p, S_dev));
    enqueue_ranking(ctx, S_dev, N, min_separation);
    return GDCA_OK;
}

gdca_status gdca_run_ranked_phased_async(gdca_ctx *const *ctxs, int32_t K, const int8_t *const *Z_host, const int32_t *N, const int32_t *M,
                                         const int32_t *q, const gdca_params *p, int32_t min_separation)
{
    if (!ctxs || K < 1 || K > 64 || !Z_host || !N || !M || !q || !p) return GDCA_EINVAL;
    gdca_ctx *lead = ctxs[0];
    if (!lead) return GDCA_EINVAL;
    gdca_ctx *ctx = lead;  // (the error macros' context)
    if (min_separation < 1) return fail(lead, GDCA_EINVAL, "min_separation < 1");
    const int8_t *Zd[64];
    double *Sd[64];
    for (int k = 0; k < K; ++k) {
        gdca_ctx *m = ctxs[k];
        if (!m || !Z_host[k]) return fail(lead, GDCA_EINVAL, "null context or alignment in the batch");
        gdca_status vs = validate(m, N[k], M[k], q[k]);
        if (vs == GDCA_OK) vs = not_pending(m);
        if (vs != GDCA_OK) return member_error(lead, m, k, vs);
    }
    HIPCHK(hipSetDevice(lead->device));
    for (int k = 0; k < K; ++k) {
        gdca_ctx *m = ctxs[k];
        // (each member's upload goes to its own stream; gdca_run_dev_phased waits for the members' streams before it enqueues
        // anything, and the leader's upload sits on the very stream the batch is enqueued on)
        host_stage sg(m);
        Zd[k] = sg.in(Z_host[k], (size_t)N[k] * M[k]);
        Sd[k] = (double *)sg.room((size_t)N[k] * N[k] * sizeof(double));
        if (sg.status() != GDCA_OK) return member_error(lead, m, k, sg.status());
    }
    // Z_host may be released when this call returns (gdca.h): from pageable memory the copies above are complete by now, from
    // pinned or registered memory they are true DMAs still in flight -- wait for every one of them HERE, whatever path the call
    // takes afterwards (gdca_run_dev_phased synchronises the members' streams too, but not on its early argument checks)
    CHK(upload_done(lead));
    for (int k = 1; k < K; ++k)
        if (hipStreamSynchronize(ctxs[k]->stream) != hipSuccess) return fail(lead, GDCA_EHIP, "upload of a member's alignment");
    bool ranked = false;  // (issued as batched grids, the rankings are part of the batch)
    CHK(run_phased(ctxs, K, Zd, N, M, q, p, Sd, min_separation, &ranked));
    // every member's ranking behind its scores, on the member's own stream (which now waits for the batch)
    for (int k = 0; k < K && !ranked; ++k) enqueue_ranking(ctxs[k], Sd[k], N[k], min_separation);
    return GDCA_OK;
}

gdca_status gdca_run_ranked_collect(gdca_ctx *ctx, int32_t *i_out, int32_t *j_out, double *score_out, gdca_stats *st)
{
    if (!ctx) return GDCA_EINVAL;
    auto &r = ctx->pend.rank;
    if (!r.pending) return fail(ctx, GDCA_EINVAL, "no enqueued ranked run to collect");
    r.pending = false;
    gdca_stats own;
    CHK(gdca_run_collect(ctx, st ? st : &own));
    if (r.status != GDCA_OK) return r.status;
    if (r.len == 0) return GDCA_OK;
    if (!i_out || !j_out || !score_out) return fail(ctx, GDCA_EINVAL, "null pointer");
    // (a run whose inverse was refined, recomputed or run again at collect time has new scores: rank those)
    if (ctx->pend.at.refined != 0 || ctx->pend.at.rescored)
        CHK(ranking_stage(ctx, ctx->pend.target.out, ctx->pend.N, r.sep, r.len, &r.i, &r.j, &r.s));
    return ranking_to_host(ctx, r.len, r.i, r.j, r.s, i_out, j_out, score_out);
}

gdca_status gdca_run_ranked(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t min_separation,
                            int32_t *i_out, int32_t *j_out, double *score_out, gdca_stats *st)
{
    if (ctx && gdca_ranking_length(N, min_separation) > 0 && (!i_out || !j_out || !score_out)) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(gdca_run_ranked_async(ctx, Z_host, N, M, q, p, min_separation));
    return gdca_run_ranked_collect(ctx, i_out, j_out, score_out, st);
}

}  // extern "C"

// ---- several pseudocount / score settings of one alignment (gdca_run_multi, include/gdca.h) -------------------------------------
// Only the pseudocount and what follows it depend on the setting: theta, the reweighting, Pi and the pair tallies run ONCE, the pair
// tallies in their Pij_true form (k_pair_tally mode 0) into ctx->Pij.  Then for every distinct pseudocount, in order of first
// appearance (a "group"): the covariance from Pij_true (k_cov_from_pij: bit for bit the fused build of that pseudocount), the DI
// diagonal blocks if a member asks for DI, the inverse -- collected for the group's first member exactly like a single run (second
// attempt, refinement, Cholesky fallback: each builds C again from Pij_true, rebuild_padded) -- and every further member scored
// from the inverse the collect left.  A single run of any member would compute the same C, the same inverse and the same scores.
struct multi_rank {
    int sep;
    long long len;
    int32_t *i_out, *j_out;
    double *score_out;
};

// every member as run_check_args checks a single run, and one theta setting (equal, or all negative: :auto) -- before anything is enqueued
static gdca_status multi_check_args(gdca_ctx *ctx, const void *Z, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K, double *S)
{
    if (!ctx) return GDCA_EINVAL;
    if (K < 1 || K > GDCA_MULTI_MAX) return fail(ctx, GDCA_EINVAL, "number of settings must be between 1 and GDCA_MULTI_MAX");
    if (!p) return fail(ctx, GDCA_EINVAL, "null pointer");
    for (int k = 0; k < K; ++k) {
        CHK(run_check_args(ctx, (const int8_t *)Z, N, M, q, &p[k], S));
        if (!(p[k].theta == p[0].theta || (p[k].theta < 0.0 && p[0].theta < 0.0)))
            return fail(ctx, GDCA_EINVAL, "every setting of one call must have the same theta");
    }
    return not_pending(ctx);
}

static gdca_status multi_rank_member(gdca_ctx *ctx, const multi_rank *rk, int k, const double *S_dev)
{
    if (rk->len == 0) return GDCA_OK;
    int32_t *ii, *jj;
    double *sv;
    CHK(ranking_stage(ctx, S_dev, ctx->pend.N, rk->sep, rk->len, &ii, &jj, &sv));
    const size_t at = (size_t)k * (size_t)rk->len;
    return ranking_to_host(ctx, rk->len, ii, jj, sv, rk->i_out + at, rk->j_out + at, rk->score_out + at);
}

// K >= 2 members, arguments checked.  Member k's scores go to S_dev + k S_stride (S_stride 0: one matrix, ranked before the next
// member overwrites it); st: K entries
static gdca_status run_multi(gdca_ctx *ctx, const int8_t *Z_dev, int N, int M, int q, const gdca_params *p, int K, double *S_dev, size_t S_stride,
                             gdca_stats *st, const multi_rank *rk)
{
    hipStream_t s = ctx->stream;
    const int sdim = q - 1, n = N * sdim, n_pad = round_up(n, GDCA_TILE);
    gdca_status mst[GDCA_MULTI_MAX];
    bool done[GDCA_MULTI_MAX];
    double ldv[GDCA_MULTI_MAX];  // every member's log det (its group's) and where it came from: the context's record when the call returns
    int lds[GDCA_MULTI_MAX];
    for (int k = 0; k < K; ++k) {
        memset(&st[k], 0, sizeof(st[k]));
        mst[k] = GDCA_OK;
        done[k] = false;
        ldv[k] = (double)NAN;
        lds[k] = 0;
    }
    // ---- the front end, once: theta, reweighting, Pi, Pij_true (ld = n) ----
    CHK(front_weights(ctx, Z_dev, N, M, q, p[0].theta, false));
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    CHK(ensure(ctx, ctx->Pij, (size_t)n * n * sizeof(double)));
    CHK(ensure(ctx, ctx->A, (size_t)n_pad * n_pad * sizeof(double)));
    CHK(ensure(ctx, ctx->sc_front, sizeof(gdca_dev_scalars)));
    CHK(tally_stage(ctx, Z_dev, N, M, q, &sc->Meff, p[0].pseudocount, 0, nullptr, (double *)ctx->Pij.p, (size_t)n));
    HIPCHK(hipMemcpyAsync(ctx->sc_front.p, sc, sizeof(gdca_dev_scalars), hipMemcpyDeviceToDevice, s));
    pending_front(ctx, Z_dev, N, M, q, &p[0], (const double *)ctx->Pij.p);
    double ms_theta = 0.0, ms_weights = 0.0;
    bool first = true;
    for (int k0 = 0; k0 < K; ++k0) {
        if (done[k0]) continue;
        // ---- the group of p[k0].pseudocount: covariance, DI blocks, inverse; its first member collected like a single run ----
        const double pc = p[k0].pseudocount;
        bool di = false;
        for (int k = k0; k < K; ++k) di = di || (p[k].pseudocount == pc && p[k].score == GDCA_SCORE_DI);
        if (!first) {
            // (every group starts from the scalars the front end left: theta, Meff, ...; its own -- pi_max, norms, info -- zero)
            HIPCHK(hipMemcpyAsync(sc, ctx->sc_front.p, sizeof(gdca_dev_scalars), hipMemcpyDeviceToDevice, s));
            ctx->pend.at = gdca_pending::progress{};
            CHK(mark(ctx, T_WEIGHTS));
        }
        ctx->pend.p = p[k0];
        CHK(cov_from_pij_stage(ctx, N, M, q, pc, (double *)ctx->A.p, (size_t)n_pad, ctx->tune.refine != 0));
        CHK(covariance_tail(ctx, N, sdim, n_pad, di));
        CHK(run_inverse(ctx));
        double *S0 = S_dev + (size_t)k0 * S_stride;
        CHK(run_score(ctx, contact_target(p[k0].score, p[k0].apc, S0)));
        const gdca_status gs = gdca_run_collect(ctx, &st[k0]);
        if (gs == GDCA_EHIP || gs == GDCA_ENOMEM || gs == GDCA_EINVAL) return gs;  // (EINVAL here: a symbol outside 1..q)
        mst[k0] = gs;
        done[k0] = true;
        ldv[k0] = ctx->ld.val[0];
        lds[k0] = ctx->ld.src[0];
        if (first) {
            ms_theta = st[k0].ms_theta;
            ms_weights = st[k0].ms_weights;
            first = false;
        } else {
            st[k0].ms_theta = ms_theta;
            st[k0].ms_weights = ms_weights;
        }
        if (gs == GDCA_OK && rk) CHK(multi_rank_member(ctx, rk, k0, S0));
        // ---- the group's further members: scored from the inverse the collect left in ctx->A ----
        const int ginfo = ctx->sc_host->info;  // the group's: 0, or the leading minor that is not positive definite
        for (int k = k0 + 1; k < K; ++k) {
            if (done[k] || p[k].pseudocount != pc) continue;
            done[k] = true;
            ldv[k] = ldv[k0];
            lds[k] = lds[k0];
            st[k] = st[k0];
            st[k].info = ginfo;
            st[k].ms_fn = 0.0;
            st[k].ms_score = 0.0;
            if (ginfo != 0) {
                mst[k] = GDCA_ENOTPD;
                continue;
            }
            double *Sk = S_dev + (size_t)k * S_stride;
            ctx->pend.target = contact_target(p[k].score, p[k].apc, Sk);
            CHK(rescore(ctx, true));
            CHK(score_times(ctx, &st[k]));
            if (ctx->sc_host->di_noconv != 0) {
                st[k].info = -ctx->sc_host->di_noconv;
                mst[k] = fail(ctx, GDCA_ENOCONV, GDCA_TEXT_DI_NOCONV);
                continue;
            }
            if (rk) CHK(multi_rank_member(ctx, rk, k, Sk));
        }
    }
    for (int k = 0; k < K; ++k) {
        ctx->ld.val[k] = ldv[k];
        ctx->ld.src[k] = lds[k];
    }
    ctx->ld.count = K;
    for (int k = 0; k < K; ++k)
        if (mst[k] != GDCA_OK) {
            char msg[sizeof(ctx->err)];
            snprintf(msg, sizeof(msg), "setting %d: %s", k, mst[k] == GDCA_ENOTPD ? GDCA_TEXT_COV_NOT_PD : GDCA_TEXT_DI_NOCONV);
            memcpy(ctx->err, msg, sizeof(msg));
            return mst[k];
        }
    return GDCA_OK;
}

extern "C" {

gdca_status gdca_run_multi_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K,
                               double *S_dev, gdca_stats *st)
{
    CHK(multi_check_args(ctx, Z_dev, N, M, q, p, K, S_dev));
    if (K == 1) return gdca_run_dev(ctx, Z_dev, N, M, q, p, S_dev, st);
    gdca_stats own[GDCA_MULTI_MAX];
    return run_multi(ctx, Z_dev, N, M, q, p, K, S_dev, (size_t)N * N, st ? st : own, nullptr);
}

gdca_status gdca_run_multi(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K,
                           double *S_host, gdca_stats *st)
{
    CHK(multi_check_args(ctx, Z_host, N, M, q, p, K, S_host));
    if (K == 1) return gdca_run(ctx, Z_host, N, M, q, p, S_host, st);
    const size_t mat = (size_t)N * N;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    double *S_dev = sg.out(S_host, (size_t)K * mat * sizeof(double));
    CHK(sg.status());
    gdca_stats own[GDCA_MULTI_MAX];
    const gdca_status rs = run_multi(ctx, Z_dev, N, M, q, p, K, S_dev, mat, st ? st : own, nullptr);
    if (rs != GDCA_OK && rs != GDCA_ENOTPD && rs != GDCA_ENOCONV) return rs;
    // (the members that did not fail are results: all K blocks come back)
    CHK(sg.finish(GDCA_OK));
    return rs;
}

gdca_status gdca_run_ranked_multi(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t K,
                                  int32_t min_separation, int32_t *i_out, int32_t *j_out, double *score_out, gdca_stats *st)
{
    if (!ctx) return GDCA_EINVAL;
    if (min_separation < 1) return fail(ctx, GDCA_EINVAL, "min_separation < 1");
    double placeholder = 0.0;  // (no score matrix crosses this ABI: the one the members share is the context's)
    CHK(multi_check_args(ctx, Z_host, N, M, q, p, K, &placeholder));
    const long long len = gdca_ranking_length(N, min_separation);
    if (len > 0 && (!i_out || !j_out || !score_out)) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (K == 1) return gdca_run_ranked(ctx, Z_host, N, M, q, p, min_separation, i_out, j_out, score_out, st);
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    double *S_dev = (double *)sg.room((size_t)N * N * sizeof(double));  // (the one matrix the members share)
    CHK(sg.status());
    const multi_rank rk{min_separation, len, i_out, j_out, score_out};
    gdca_stats own[GDCA_MULTI_MAX];
    return run_multi(ctx, Z_dev, N, M, q, p, K, S_dev, 0, st ? st : own, &rk);
}

// ---- caller-visible device buffers ----------------------------------------------------------------------
// A gdca_dbuf is nothing but an owned HBM allocation: the `_dev` operators below take plain device pointers
// (gdca_dbuf_ptr of such a buffer, or any other device memory of the same GPU, e.g. a torch tensor's data_ptr).

struct gdca_dbuf {
    void *p;
    size_t bytes;
    int device;
};

gdca_status gdca_dbuf_alloc(gdca_ctx *ctx, uint64_t bytes, gdca_dbuf **out)
{
    if (!ctx || !out) return GDCA_EINVAL;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    gdca_dbuf *b = (gdca_dbuf *)calloc(1, sizeof(gdca_dbuf));
    if (!b) return GDCA_ENOMEM;
    const size_t want = bytes ? (size_t)bytes : 16;
    hipError_t e = hipMalloc(&b->p, want);
    if (e != hipSuccess) {
        free(b);
        (void)hipGetLastError();
        return fail(ctx, GDCA_ENOMEM, "hipMalloc failed: %s%s", hipGetErrorString(e), "");
    }
    b->bytes = want;
    b->device = ctx->device;
    *out = b;
    return GDCA_OK;
}

gdca_status gdca_dbuf_free(gdca_dbuf *b)
{
    if (!b) return GDCA_OK;
    (void)hipSetDevice(b->device);
    if (b->p) (void)hipFree(b->p);
    free(b);
    return GDCA_OK;
}

void *gdca_dbuf_ptr(const gdca_dbuf *b)
{
    return b ? b->p : nullptr;
}

uint64_t gdca_dbuf_bytes(const gdca_dbuf *b)
{
    return b ? (uint64_t)b->bytes : 0;
}

gdca_status gdca_dbuf_upload(gdca_ctx *ctx, gdca_dbuf *b, uint64_t offset, const void *host, uint64_t bytes)
{
    if (!ctx || !b || (!host && bytes) || offset + bytes > b->bytes) return GDCA_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes) HIPCHK(hipMemcpyAsync((char *)b->p + offset, host, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the host buffer may be reused on return
    return GDCA_OK;
}

gdca_status gdca_dbuf_download(gdca_ctx *ctx, const gdca_dbuf *b, uint64_t offset, void *host, uint64_t bytes)
{
    if (!ctx || !b || (!host && bytes) || offset + bytes > b->bytes) return GDCA_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes) HIPCHK(hipMemcpyAsync(host, (const char *)b->p + offset, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

gdca_status gdca_dbuf_copy(gdca_ctx *ctx, gdca_dbuf *dst, const gdca_dbuf *src, uint64_t bytes)
{
    if (!ctx || !dst || !src || bytes > dst->bytes || bytes > src->bytes) return GDCA_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes && dst->p != src->p) HIPCHK(hipMemcpyAsync(dst->p, src->p, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return GDCA_OK;
}

// ---- operator level, device-resident (`_dev`): every matrix argument is a device pointer ----------------------
// Each call enqueues on the ctx stream and returns after the stream has drained only where a host scalar comes
// back (weights: Meff/theta/thresh; spd_inverse: info; di: convergence; frequencies: the symbol-range check); the
// elementwise ones (add_pseudocount, covariance, fn, apc) return right after the launch.

gdca_status gdca_pair_identity_sum_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, uint64_t *out)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z_dev || !out) return GDCA_EINVAL;
    CHK(begin(ctx));
    CHK(weights_stage(ctx, Z_dev, N, M, GDCA_MAXQ, -1.0, -1, true));
    CHK(fetch_scalars(ctx));
    *out = ctx->sc_host->pair_sum;
    return GDCA_OK;
}

gdca_status gdca_compute_theta_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, double *theta)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z_dev || !theta) return GDCA_EINVAL;
    CHK(begin(ctx));
    CHK(weights_stage(ctx, Z_dev, N, M, GDCA_MAXQ, -1.0, -1, true));
    CHK(fetch_scalars(ctx));
    *theta = ctx->sc_host->theta;
    return GDCA_OK;
}

gdca_status gdca_neighbour_counts_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t thresh,
                                      int32_t *n_dev)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z_dev || !n_dev || thresh < 0) return GDCA_EINVAL;
    CHK(begin(ctx));
    CHK(weights_stage(ctx, Z_dev, N, M, GDCA_MAXQ, 0.0, thresh, false));
    HIPCHK(hipMemcpyAsync(n_dev, ctx->nk.p, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    CHK(fetch_scalars(ctx));
    return conclude(ctx, GDCA_ENDS_FRONT);
}

gdca_status gdca_compute_weights_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, double theta,
                                     double *W_dev, double *Meff, double *theta_used, int32_t *thresh)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z_dev || !W_dev || !Meff || !(theta <= 1.0)) return GDCA_EINVAL;
    CHK(begin(ctx));
    CHK(weights_stage(ctx, Z_dev, N, M, GDCA_MAXQ, theta, -1, false));
    HIPCHK(hipMemcpyAsync(W_dev, ctx->W.p, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    CHK(fetch_scalars(ctx));
    *Meff = ctx->sc_host->Meff;
    if (theta_used) *theta_used = ctx->sc_host->theta;
    if (thresh) *thresh = ctx->sc_host->thresh;
    return conclude(ctx, GDCA_ENDS_FRONT);
}

gdca_status gdca_frequencies_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q,
                                 const double *W_dev, double Meff, double *Pi_dev, double *Pij_dev)
{
    CHK(validate(ctx, N, M, q));
    if (!Z_dev || !W_dev || !Pi_dev || !Pij_dev || !(Meff > 0.0)) return GDCA_EINVAL;
    CHK(begin(ctx));
    hipStream_t s = ctx->stream;
    const int sdim = q - 1, n = N * sdim;
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    CHK(ensure(ctx, ctx->Wfix, (size_t)M * sizeof(unsigned long long)));
    // Meff travels through the device scalar block (the tally kernels read it from HBM)
    HIPCHK(hipMemcpyAsync(&sc->Meff, &Meff, sizeof(double), hipMemcpyHostToDevice, s));
    // W outside [0, 1] would overflow the 59-bit fixed-point weight field: flagged on the device
    gdca_launch_fix_weights(s, W_dev, M, gdca_fix_shift(M), (unsigned long long *)ctx->Wfix.p, sc);
    CHK(tally_stage(ctx, Z_dev, N, M, q, &sc->Meff, 0.0, 0, Pi_dev, Pij_dev, (size_t)n));
    CHK(fetch_scalars(ctx));
    if (ctx->sc_host->bad_symbol & GDCA_BAD_WEIGHT) return fail(ctx, GDCA_EINVAL, "weights must lie in [0, 1]");
    return conclude(ctx, GDCA_ENDS_FRONT);
}

gdca_status gdca_add_pseudocount_dev(gdca_ctx *ctx, const double *Pi_true_dev, const double *Pij_true_dev, int32_t N,
                                     int32_t q, double pc, double *Pi_dev, double *Pij_dev)
{
    CHK(validate(ctx, N, 1, q));
    if (!Pi_true_dev || !Pij_true_dev || !Pi_dev || !Pij_dev || !(pc >= 0.0 && pc <= 1.0)) return GDCA_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    gdca_launch_add_pseudocount(ctx->stream, Pi_true_dev, Pij_true_dev, N, q, pc, Pi_dev, Pij_dev);
    return check_launch(ctx, "add_pseudocount");
}

gdca_status gdca_covariance_dev(gdca_ctx *ctx, const double *Pi_dev, const double *Pij_dev, int32_t n, double *C_dev)
{
    if (!ctx || !Pi_dev || !Pij_dev || !C_dev || n < 1 || n > GDCA_MAX_N) return GDCA_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    gdca_launch_covariance(ctx->stream, Pi_dev, Pij_dev, n, C_dev);
    return check_launch(ctx, "covariance");
}

// The operator-level inverse of the caller's matrix: a first attempt is enqueued on the context's stream (its matrix copied into ctx->A,
// pend.n / pend.n_pad set) -- the log det of its pivots behind it, the scalars fetched, the ladder with up to `retries` further
// attempts, and the result copied out.  Not where the watchdog had the last word: the caller's matrix stays as it is.
static gdca_status operator_ladder(gdca_ctx *ctx, double *A_dev, int retries, bool first)
{
    if (first) {
        CHK(logdet_stage(ctx, ctx->pend.n));
        CHK(fetch_scalars(ctx));
    }
    CHK(inverse_ladder(ctx, inverse_source{GDCA_FORM_OPERATOR, A_dev}, retries));
    if (ctx->sc_host->info == GDCA_INFO_WATCHDOG) return GDCA_OK;
    gdca_launch_copy_out_neg_sym(ctx->stream, (const double *)ctx->A.p, ctx->pend.n_pad, A_dev, ctx->pend.n);
    CHK(check_launch(ctx, "copy_out"));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

static gdca_status operator_copy_in(gdca_ctx *ctx, const double *A_dev, int n)
{
    const int n_pad = round_up(n, GDCA_TILE);
    CHK(begin(ctx));
    CHK(ensure(ctx, ctx->A, (size_t)n_pad * n_pad * sizeof(double)));
    gdca_launch_copy_in(ctx->stream, A_dev, n, (double *)ctx->A.p, n_pad);
    ctx->pend.n = n;
    ctx->pend.n_pad = n_pad;
    return GDCA_OK;
}

gdca_status gdca_spd_inverse_dev(gdca_ctx *ctx, double *A_dev, int32_t n, int32_t *info)
{
    if (!ctx || !A_dev || n < 1 || n > GDCA_MAX_N) return GDCA_EINVAL;
    CHK(operator_copy_in(ctx, A_dev, n));
    CHK(inverse_stage(ctx, n, ctx->pend.n_pad, nullptr));
    CHK(operator_ladder(ctx, A_dev, ctx->tune.sweep_retries, true));
    note_logdet(ctx);
    if (info) *info = ctx->sc_host->info == GDCA_INFO_WATCHDOG ? 0 : ctx->sc_host->info;
    return conclude(ctx, GDCA_ENDS_INVERSE);
}

gdca_status gdca_spd_inverse_batch_dev(gdca_ctx *const *ctxs, int32_t K, double *const *A_dev, const int32_t *n, int32_t *info)
{
    if (!ctxs || K < 1 || K > 64 || !A_dev || !n) return GDCA_EINVAL;
    gdca_ctx *lead = ctxs[0];
    if (!lead) return GDCA_EINVAL;
    gdca_ctx *ctx = lead;
    for (int k = 0; k < K; ++k) {
        if (!ctxs[k] || !A_dev[k] || n[k] < 1 || n[k] > GDCA_MAX_N) return fail(lead, GDCA_EINVAL, "invalid member of the batch");
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return fail(lead, GDCA_EINVAL, "the same context twice in one batch");
        if (ctxs[k]->device != lead->device) return fail(lead, GDCA_EINVAL, "contexts of one batch must share a device");
        CHK(not_pending(ctxs[k]));
        if (info) info[k] = 0;
    }
    HIPCHK(hipSetDevice(lead->device));
    hipStream_t own[64];
    for (int k = 0; k < K; ++k) {
        own[k] = ctxs[k]->stream;
        if (k > 0) (void)hipStreamSynchronize(own[k]);
        ctxs[k]->stream = lead->stream;
    }
    gdca_status st = GDCA_OK;
    for (int k = 0; k < K && st == GDCA_OK; ++k) st = member_error(lead, ctxs[k], k, operator_copy_in(ctxs[k], A_dev[k], n[k]));
    if (st == GDCA_OK) st = run_inverses(lead, ctxs, K);
    // the ladder member by member on the leader's stream, as gdca_spd_inverse_dev walks it (the caller's matrices are still intact; each
    // member's switches are its own context's) -- but for the further attempts of a launch the watchdog ended: see below
    for (int k = 0; k < K && st == GDCA_OK; ++k) st = member_error(lead, ctxs[k], k, operator_ladder(ctxs[k], A_dev[k], 0, true));
    (void)hipStreamSynchronize(lead->stream);
    for (int k = 0; k < K; ++k) ctxs[k]->stream = own[k];
    // members whose launch the watchdog ended (all members of a merged launch share that fate): once more, one by one, each on its own stream
    for (int k = 0; k < K && st == GDCA_OK; ++k) {
        gdca_ctx *m = ctxs[k];
        if (m->sc_host->info == GDCA_INFO_WATCHDOG) st = member_error(lead, m, k, operator_ladder(m, A_dev[k], m->tune.sweep_retries, false));
    }
    if (st != GDCA_OK) return st;
    gdca_verdict worst{GDCA_OK, nullptr};
    for (int k = 0; k < K; ++k) {
        note_logdet(ctxs[k]);
        const int inf = ctxs[k]->sc_host->info;
        const gdca_verdict v = gdca_verdict_of(GDCA_ENDS_INVERSE, 0, inf, 0);
        if (v.status == GDCA_ENOTPD && info) info[k] = inf;
        worst = gdca_worse_verdict(worst, v);
    }
    return worst.status == GDCA_OK ? GDCA_OK : fail(lead, worst.status, worst.text);
}

// mJ (device, n x n full, ld n) -> ctx->A as "-mJ" with ld = n_pad (the score kernels read its lower triangle)
static gdca_status stage_neg_mJ(gdca_ctx *ctx, const double *mJ_dev, int n, int n_pad)
{
    CHK(ensure(ctx, ctx->A, (size_t)n_pad * n_pad * sizeof(double)));
    gdca_launch_copy_in_neg(ctx->stream, mJ_dev, n, (double *)ctx->A.p, n_pad);
    return check_launch(ctx, "stage_mJ");
}

gdca_status gdca_fn_dev(gdca_ctx *ctx, const double *mJ_dev, int32_t N, int32_t q, double *S_dev)
{
    CHK(validate(ctx, N, 1, q));
    if (!mJ_dev || !S_dev) return GDCA_EINVAL;
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    ctx->pend.timed = false;  // (no scalars, so no begin(): the timeline of the context's last run is closed here)
    const int sdim = q - 1, n = N * sdim, n_pad = round_up(n, GDCA_TILE);
    CHK(stage_neg_mJ(ctx, mJ_dev, n, n_pad));
    return score_stage(ctx, N, sdim, n_pad, contact_target(GDCA_SCORE_FROB, 0, S_dev));
}

gdca_status gdca_di_dev(gdca_ctx *ctx, const double *mJ_dev, const double *C_dev, int32_t N, int32_t q, double *S_dev)
{
    CHK(validate(ctx, N, 1, q));
    if (!mJ_dev || !C_dev || !S_dev) return GDCA_EINVAL;
    CHK(begin(ctx));
    hipStream_t s = ctx->stream;
    const int sdim = q - 1, n = N * sdim, n_pad = round_up(n, GDCA_TILE);
    CHK(ensure(ctx, ctx->Dblk, (size_t)N * sdim * sdim * sizeof(double)));
    CHK(ensure(ctx, ctx->Ld, (size_t)N * sdim * sdim * sizeof(double)));
    gdca_launch_save_diag_blocks(s, C_dev, (size_t)n, N, sdim, (double *)ctx->Dblk.p);
    gdca_launch_diag_chol(s, (const double *)ctx->Dblk.p, N, sdim, (double *)ctx->Ld.p);
    CHK(stage_neg_mJ(ctx, mJ_dev, n, n_pad));
    CHK(score_stage(ctx, N, sdim, n_pad, contact_target(GDCA_SCORE_DI, 0, S_dev)));
    CHK(fetch_scalars(ctx));
    if (ctx->sc_host->di_noconv)
        return fail(ctx, GDCA_ENOCONV, GDCA_TEXT_DI_NOCONV);
    return GDCA_OK;
}

// ---- the model read-outs: operator forms (the caller's mJ_dev / Pi_dev) and fused forms (run_target) ----
// an operator's model: mJ itself, dense n x n
static gdca_model operator_model(const double *mJ_dev, const double *Pi_dev, int N, int q)
{
    return gdca_model{mJ_dev, (size_t)N * (q - 1), 1.0, Pi_dev, N, q};
}

// how the operator forms end: the stage's flags fetched, an illegal byte among the sequences reported
static gdca_status sequences_checked(gdca_ctx *ctx)
{
    CHK(fetch_scalars(ctx));
    return conclude(ctx, GDCA_ENDS_READOUT);
}

// the fused form of the energy entries, their own arguments checked: gdca_run's front end and inverse, then the stage `t` names in
// the place of the contact score, collected at once
static gdca_status run_target(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, const score_target &t,
                              gdca_stats *st)
{
    CHK(check_params(ctx, p));
    CHK(not_pending(ctx));
    gdca_params pp = *p;  // (score and apc are ignored: no contact score is computed)
    pp.score = GDCA_SCORE_FROB;
    pp.apc = 0;
    CHK(run_front(ctx, Z_dev, N, M, q, &pp));
    CHK(run_inverse(ctx));
    CHK(run_score(ctx, t));
    return gdca_run_collect(ctx, st);
}

// The argument checks of an entry point with more to check than one condition: one text for its `_dev` form and its host-pointer form
// (a pointer is only compared with nullptr, so device and host pointers are checked alike) -- the check_* functions here and further
// down, beside validate_concat and ipa_check.  Nothing has run, and nothing is staged, when one fails.
static gdca_status check_energies(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *X, int K, const void *E)
{
    CHK(validate(ctx, N, K, q));
    if (!mJ || !Pi || !X || !E) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

static gdca_status check_run_energies(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, const void *X, int K,
                                      const void *E)  // ... and gdca_run_loglik
{
    CHK(validate(ctx, N, M, q));
    if (!Z || !E || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (X && K < 1) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    return GDCA_OK;
}

gdca_status gdca_energies_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev, int32_t K,
                              double *E_dev)
{
    CHK(check_energies(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, E_dev));
    CHK(begin(ctx));
    CHK(energy_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), X_dev, K, E_dev));
    return sequences_checked(ctx);
}

gdca_status gdca_run_energies_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                  const int8_t *X_dev, int32_t K, double *E_dev, gdca_stats *st)
{
    CHK(check_run_energies(ctx, Z_dev, N, M, q, p, X_dev, K, E_dev));
    return run_target(ctx, Z_dev, N, M, q, p, energy_target(Z_dev, M, X_dev, K, E_dev), st);
}

gdca_status gdca_last_logdet(gdca_ctx *ctx, int32_t k, double *logdet, int32_t *source)
{
    if (!ctx) return GDCA_EINVAL;
    if (!logdet) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(not_pending(ctx));
    if (ctx->ld.count == 0) return fail(ctx, GDCA_EINVAL, "no SPD inverse has been completed on this context");
    if (k < 0 || k >= ctx->ld.count) return fail(ctx, GDCA_EINVAL, "member index out of range");
    *logdet = ctx->ld.val[k];
    if (source) *source = ctx->ld.src[k];
    return GDCA_OK;
}

gdca_status gdca_spd_inverse_logdet_dev(gdca_ctx *ctx, double *A_dev, int32_t n, int32_t *info, double *logdet)
{
    if (!ctx || !logdet) return GDCA_EINVAL;
    *logdet = (double)NAN;
    const gdca_status st = gdca_spd_inverse_dev(ctx, A_dev, n, info);
    if (ctx->ld.count > 0 && !ctx->pending) *logdet = ctx->ld.val[0];
    return st;
}

gdca_status gdca_run_loglik_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                const int8_t *X_dev, int32_t K, double *L_dev, double *logdet, gdca_stats *st)
{
    CHK(check_run_energies(ctx, Z_dev, N, M, q, p, X_dev, K, L_dev));
    if (logdet) *logdet = (double)NAN;
    const gdca_status rs = run_target(ctx, Z_dev, N, M, q, p, loglik_target(Z_dev, M, X_dev, K, L_dev), st);
    if (logdet && ctx->ld.count > 0 && !ctx->pending) *logdet = ctx->ld.val[0];
    return rs;
}

// the argument checks the four pair entry points share (nothing has run when one fails); KA / KB as they will be used
static gdca_status validate_pair(gdca_ctx *ctx, int N, int q, int split, long long KA, long long KB, int what)
{
    CHK(validate(ctx, N, 1, q));
    if (split < 1 || split > N - 1) return fail(ctx, GDCA_EINVAL, "invalid split (must be between 1 and N - 1)");
    if (KA < 1 || KB < 1 || KA + KB > INT32_MAX) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    if (what != GDCA_PAIR_COUPLING && what != GDCA_PAIR_ENERGY) return fail(ctx, GDCA_EINVAL, "invalid value of `what`");
    return GDCA_OK;
}

static gdca_status check_pair_energies(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, int split, const void *XA, int KA,
                                       const void *XB, int KB, int what, const void *E)  // ... and the blocked form, before its species
{
    CHK(validate_pair(ctx, N, q, split, KA, KB, what));
    if (!mJ || !XA || !XB || !E || (what == GDCA_PAIR_ENERGY && !Pi)) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

// a fused pair form: gdca_run_pair_energies, gdca_run_pair_logodds (what: GDCA_PAIR_ENERGY)
static gdca_status check_run_pair(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, int split, const void *XA, int KA,
                                  const void *XB, int KB, int what, const void *out)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_pair(ctx, N, q, split, XA ? KA : M, XB ? KB : M, what));
    if (!Z || !out || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_pair_energies_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, int32_t split,
                                   const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, int32_t what, double *E_dev)
{
    CHK(check_pair_energies(ctx, mJ_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, what, E_dev));
    CHK(begin(ctx));
    CHK(pair_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), split, XA_dev, (size_t)split, KA, XB_dev, (size_t)(N - split), KB, what, E_dev));
    return sequences_checked(ctx);
}

gdca_status gdca_run_pair_energies_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                       const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, int32_t what, double *E_dev,
                                       gdca_stats *st)
{
    CHK(check_run_pair(ctx, Z_dev, N, M, q, p, split, XA_dev, KA, XB_dev, KB, what, E_dev));
    return run_target(ctx, Z_dev, N, M, q, p, pair_target(Z_dev, N, M, split, XA_dev, KA, XB_dev, KB, what, E_dev), st);
}

// ---- partner matching per species: the blocked pair energies and the assignment ----
// eoff[S] of valid species offsets (S + 1 host int32 each: from 0, non-decreasing), or -1; *kmax: the largest kA_s or kB_s
static long long blocks_length(const int32_t *offA, const int32_t *offB, int S, int *kmax)
{
    if (!offA || !offB || S < 1 || offA[0] != 0 || offB[0] != 0) return -1;
    long long total = 0;
    int km = 0;
    for (int s = 0; s < S; ++s) {
        const long long ka = (long long)offA[s + 1] - offA[s], kb = (long long)offB[s + 1] - offB[s];
        if (ka < 0 || kb < 0) return -1;
        total += ka * kb;
        km = std::max(km, (int)std::max(ka, kb));
    }
    if (kmax) *kmax = km;
    return total;
}

int64_t gdca_pair_blocks_length(const int32_t *offA, const int32_t *offB, int32_t S)
{
    return blocks_length(offA, offB, S, nullptr);
}

// the species offsets of a call (host arrays in both forms of an entry) held against its counts; *total: the packed length
static gdca_status check_blocks(gdca_ctx *ctx, const void *offA, const void *offB, int S, long long KA, long long KB, long long *total,
                                int *kmax = nullptr)
{
    if (!offA || !offB) return fail(ctx, GDCA_EINVAL, "null pointer");
    *total = blocks_length((const int32_t *)offA, (const int32_t *)offB, S, kmax);
    if (*total < 0 || ((const int32_t *)offA)[S] != KA || ((const int32_t *)offB)[S] != KB)
        return fail(ctx, GDCA_EINVAL, "invalid species offsets (S >= 1; from 0, non-decreasing, up to the number of sequences)");
    return GDCA_OK;
}

static gdca_status check_assign_blocks(gdca_ctx *ctx, const void *E, const void *offA, const void *offB, int S, const void *match)
{
    if (!ctx) return GDCA_EINVAL;
    if (!E || !offA || !offB || !match) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (S < 1) return fail(ctx, GDCA_EINVAL, "invalid species offsets (S >= 1)");
    return GDCA_OK;
}

// a fused partner form: gdca_run_partner_match, gdca_run_partner_logodds (what: GDCA_PAIR_ENERGY); ka / kb: the pools as they will be used
static gdca_status check_run_partner(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, int split, int ka, int kb,
                                     const void *offA, const void *offB, int what, const void *match)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_pair(ctx, N, q, split, ka, kb, what));
    if (!Z || !match || !offA || !offB || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

// The species of a call: offsets checked against the counts (nothing has run when that fails), the table in ctx->PBtab and -- nB > 0:
// the blocked gather will run over (N - split)(q - 1) = nB rows -- its work list in ctx->PBitems, cut at the chunks pair_stage will
// make.  `first` is the caller's: blk->first points into it.
static gdca_status species_blocks(gdca_ctx *ctx, const void *offA_, const void *offB_, int S, long long KA, long long KB, int nB, bool assign,
                                  pair_blocks *blk, std::vector<long long> &first)
{
    const int32_t *offA = (const int32_t *)offA_, *offB = (const int32_t *)offB_;
    int kmax = 0;
    long long total = 0;
    CHK(check_blocks(ctx, offA, offB, S, KA, KB, &total, &kmax));
    if (assign && kmax > GDCA_ASSIGN_MAX) return fail(ctx, GDCA_EINVAL, "a species has more than GDCA_ASSIGN_MAX sequences on one side");
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t S1 = (size_t)S + 1;
    std::vector<long long> eoff(S1, 0);
    for (int s = 0; s < S; ++s) eoff[s + 1] = eoff[s] + ((long long)offA[s + 1] - offA[s]) * ((long long)offB[s + 1] - offB[s]);
    CHK(ensure(ctx, ctx->PBtab, S1 * (sizeof(long long) + 2 * sizeof(int32_t))));
    char *tab = (char *)ctx->PBtab.p;
    HIPCHK(hipMemcpyAsync(tab, eoff.data(), S1 * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(tab + S1 * sizeof(long long), offA, S1 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(tab + S1 * (sizeof(long long) + sizeof(int32_t)), offB, S1 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    blk->eoff = (const long long *)tab;
    blk->offA = (const int32_t *)(tab + S1 * sizeof(long long));
    blk->offB = blk->offA + S1;
    blk->items = nullptr;
    blk->first = nullptr;
    blk->S = S;
    blk->Ac = 0;
    blk->kmax = kmax;
    blk->total = total;
    std::vector<int32_t> items;
    if (nB > 0) {
        blk->Ac = gdca_pair_chunk(nB, (int)KA, ctx->tune.pair_chunk);
        gdca_pair_block_items(offA, offB, S, blk->Ac, items, first);
        CHK(ensure(ctx, ctx->PBitems, items.size() * sizeof(int32_t)));
        if (!items.empty())
            HIPCHK(hipMemcpyAsync(ctx->PBitems.p, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        blk->items = (const int32_t *)ctx->PBitems.p;
        blk->first = first.data();
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));  // (the host arrays of this frame have been read)
    return GDCA_OK;
}

gdca_status gdca_pair_energies_blocked_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, int32_t split,
                                           const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, const void *offA,
                                           const void *offB, int32_t S, int32_t what, double *E_dev)
{
    CHK(check_pair_energies(ctx, mJ_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, what, E_dev));
    pair_blocks blk;
    std::vector<long long> first;
    CHK(species_blocks(ctx, offA, offB, S, KA, KB, (N - split) * (q - 1), false, &blk, first));
    CHK(begin(ctx));
    CHK(pair_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), split, XA_dev, (size_t)split, KA, XB_dev, (size_t)(N - split), KB, what, E_dev,
                   &blk));
    return sequences_checked(ctx);
}

gdca_status gdca_assign_blocks_dev(gdca_ctx *ctx, const double *E_dev, const void *offA, const void *offB, int32_t S, int32_t *match_dev,
                                   double *gap_dev)
{
    CHK(check_assign_blocks(ctx, E_dev, offA, offB, S, match_dev));
    pair_blocks blk;
    std::vector<long long> first;
    CHK(species_blocks(ctx, offA, offB, S, ((const int32_t *)offA)[S], ((const int32_t *)offB)[S], 0, true, &blk, first));
    CHK(assign_stage(ctx, E_dev, blk, match_dev, gap_dev));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

gdca_status gdca_run_partner_match_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                       const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, const void *offA, const void *offB,
                                       int32_t S, int32_t what, double *E_dev, int32_t *match_dev, double *gap_dev, gdca_stats *st)
{
    const int ka = XA_dev ? KA : M, kb = XB_dev ? KB : M;
    CHK(check_run_partner(ctx, Z_dev, N, M, q, p, split, ka, kb, offA, offB, what, match_dev));
    CHK(check_params(ctx, p));
    pair_blocks blk;
    std::vector<long long> first;
    CHK(species_blocks(ctx, offA, offB, S, ka, kb, (N - split) * (q - 1), true, &blk, first));
    if (!E_dev) {
        CHK(ensure(ctx, ctx->PBE, (size_t)blk.total * sizeof(double)));
        E_dev = (double *)ctx->PBE.p;
    }
    return run_target(ctx, Z_dev, N, M, q, p,
                      partner_target(pair_target(Z_dev, N, M, split, XA_dev, KA, XB_dev, KB, what, E_dev), blk, match_dev, gap_dev), st);
}

// ---- pair log-odds: the joint model against the two marginal models (include/gdca.h) ----
// what the operator forms share: the marginal models' energies of XA and XB into ctx->LOa / ctx->LOb (the energy stage with N = split
// and N - split, Pi's two ranges), then the pair stage's LO instances on the joint model
static gdca_status logodds_operator(gdca_ctx *ctx, const double *mJ_dev, const double *mJA_dev, const double *mJB_dev, const double *Pi_dev, int N,
                                    int q, int split, const int8_t *XA_dev, int KA, const int8_t *XB_dev, int KB, double I, double *L_dev,
                                    const pair_blocks *blk)
{
    CHK(begin(ctx));
    CHK(ensure(ctx, ctx->LOa, (size_t)KA * sizeof(double)));
    CHK(ensure(ctx, ctx->LOb, (size_t)KB * sizeof(double)));
    CHK(energy_stage(ctx, operator_model(mJA_dev, Pi_dev, split, q), XA_dev, KA, (double *)ctx->LOa.p));
    CHK(energy_stage(ctx, operator_model(mJB_dev, Pi_dev + (size_t)split * (q - 1), N - split, q), XB_dev, KB, (double *)ctx->LOb.p));
    const gdca_logodds_terms lo{(const double *)ctx->LOa.p, (const double *)ctx->LOb.p, I};
    CHK(pair_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), split, XA_dev, (size_t)split, KA, XB_dev, (size_t)(N - split), KB, GDCA_PAIR_ENERGY,
                   L_dev, blk, false, &lo));
    return sequences_checked(ctx);
}

static gdca_status check_pair_logodds(gdca_ctx *ctx, const void *mJ, const void *mJA, const void *mJB, const void *Pi, int N, int q, int split,
                                      const void *XA, int KA, const void *XB, int KB, const void *L)  // ... and the blocked form, before its species
{
    CHK(validate_pair(ctx, N, q, split, KA, KB, GDCA_PAIR_ENERGY));
    if (!mJ || !mJA || !mJB || !Pi || !XA || !XB || !L) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_pair_logodds_dev(gdca_ctx *ctx, const double *mJ_dev, const double *mJA_dev, const double *mJB_dev, const double *Pi_dev, int32_t N,
                                  int32_t q, int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, double I,
                                  double *L_dev)
{
    CHK(check_pair_logodds(ctx, mJ_dev, mJA_dev, mJB_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, L_dev));
    return logodds_operator(ctx, mJ_dev, mJA_dev, mJB_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, I, L_dev, nullptr);
}

gdca_status gdca_pair_logodds_blocked_dev(gdca_ctx *ctx, const double *mJ_dev, const double *mJA_dev, const double *mJB_dev, const double *Pi_dev,
                                          int32_t N, int32_t q, int32_t split, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB,
                                          const void *offA, const void *offB, int32_t S, double I, double *L_dev)
{
    CHK(check_pair_logodds(ctx, mJ_dev, mJA_dev, mJB_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, L_dev));
    pair_blocks blk;
    std::vector<long long> first;
    CHK(species_blocks(ctx, offA, offB, S, KA, KB, (N - split) * (q - 1), false, &blk, first));
    return logodds_operator(ctx, mJ_dev, mJA_dev, mJB_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, I, L_dev, &blk);
}

// The fused form, arguments checked: the front end once into Pij_true (gdca_run_multi's way), then three fits one after the other on the
// context's stream, each collected like a single run of its own size -- the block of sites 0 .. split - 1 with the energy stage on the A
// sequences as its target, the block of the other sites with the B sequences, and the joint fit last, whose collect ends with the pair
// stage `t` names (logodds_epilogue).  The blocks' covariances are entries of the joint one bit for bit (cov_from_pij_stage).
// EmA / EmB: where the marginal energies go (nullptr: buffers of the context).  The status is the first failing fit's.
static gdca_status run_logodds(gdca_ctx *ctx, const int8_t *Z_dev, int N, int M, int q, const gdca_params *p, score_target t, double *EmA_dev,
                               double *EmB_dev, double *info, gdca_stats *st)
{
    CHK(check_params(ctx, p));
    CHK(not_pending(ctx));
    if (info) {
        for (int i = 0; i < GDCA_LOGODDS_FIELDS; ++i) info[i] = 0.0;
        info[GDCA_LOGODDS_LOGDET] = info[GDCA_LOGODDS_LOGDET_A] = info[GDCA_LOGODDS_LOGDET_B] = info[GDCA_LOGODDS_INFORMATION] = (double)NAN;
    }
    gdca_params pp = *p;  // (score and apc are ignored: no contact score is computed)
    pp.score = GDCA_SCORE_FROB;
    pp.apc = 0;
    hipStream_t s = ctx->stream;
    const int sdim = q - 1, n = N * sdim, n_pad = round_up(n, GDCA_TILE), split = t.split;
    const double pc = pp.pseudocount;
    if (!EmA_dev) {
        CHK(ensure(ctx, ctx->LOa, (size_t)t.KA * sizeof(double)));
        EmA_dev = (double *)ctx->LOa.p;
    }
    if (!EmB_dev) {
        CHK(ensure(ctx, ctx->LOb, (size_t)t.KB * sizeof(double)));
        EmB_dev = (double *)ctx->LOb.p;
    }
    // ---- the front end, once: theta, reweighting, Pi, Pij_true (ld = n) ----
    CHK(front_weights(ctx, Z_dev, N, M, q, pp.theta, false));
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    CHK(ensure(ctx, ctx->Pij, (size_t)n * n * sizeof(double)));
    CHK(ensure(ctx, ctx->A, (size_t)n_pad * n_pad * sizeof(double)));
    CHK(ensure(ctx, ctx->sc_front, sizeof(gdca_dev_scalars)));
    CHK(mark(ctx, T_TALLY_BEGIN));  // (the tallies into Pij_true: gdca_stats.ms_pair_tally of this run, and where the first marginal fit begins)
    CHK(tally_stage(ctx, Z_dev, N, M, q, &sc->Meff, pc, 0, nullptr, (double *)ctx->Pij.p, (size_t)n));
    CHK(mark(ctx, T_TALLY_END));
    HIPCHK(hipMemcpyAsync(ctx->sc_front.p, sc, sizeof(gdca_dev_scalars), hipMemcpyDeviceToDevice, s));
    double ldv[3] = {(double)NAN, (double)NAN, (double)NAN}, ms_theta = 0.0, ms_weights = 0.0, ms_marg = 0.0;
    int lds[3] = {0, 0, 0};
    gdca_stats own;
    if (!st) st = &own;
    // ---- the fits: 1 = block A, 2 = block B, 0 = the joint one (their indices in the log-det record) ----
    const int order[3] = {1, 2, 0};
    for (int f = 0; f < 3; ++f) {
        const int k = order[f];
        const int Nf = k == 1 ? split : k == 2 ? N - split : N, site0 = k == 2 ? split : 0;
        const int nf_pad = round_up(Nf * sdim, GDCA_TILE);
        if (f > 0) {
            // (every fit starts from the scalars the front end left: theta, Meff, ...; its own -- pi_max, norms, info -- zero)
            HIPCHK(hipMemcpyAsync(sc, ctx->sc_front.p, sizeof(gdca_dev_scalars), hipMemcpyDeviceToDevice, s));
            ctx->pend.at = gdca_pending::progress{};
            CHK(mark(ctx, T_WEIGHTS));
        }
        pending_front(ctx, Z_dev, Nf, M, q, &pp, (const double *)ctx->Pij.p);
        if (k != 0) {
            ctx->pend.N_all = N;
            ctx->pend.site0 = site0;
        }
        CHK(cov_from_pij_stage(ctx, Nf, M, q, pc, (double *)ctx->A.p, (size_t)nf_pad, ctx->tune.refine != 0, ctx->pend.N_all, site0));
        CHK(covariance_tail(ctx, Nf, sdim, nf_pad, false));
        CHK(run_inverse(ctx));
        score_target tf = t;
        if (k == 0) {
            tf.logodds = true;
            tf.lo = gdca_logodds_terms{EmA_dev, EmB_dev, 0.0};
            tf.ldA = ldv[1];
            tf.ldB = ldv[2];
        } else {
            tf = score_target{};
            tf.kind = score_target::ENERGY;
            tf.out = k == 1 ? EmA_dev : EmB_dev;
            tf.X = k == 1 ? t.XA : t.XB;
            tf.strideX = k == 1 ? t.strideA : t.strideB;
            tf.K = k == 1 ? t.KA : t.KB;
        }
        CHK(run_score(ctx, tf));
        gdca_stats sf;
        const gdca_status gs = gdca_run_collect(ctx, k == 0 ? st : &sf);
        ctx->pend.N_all = ctx->pend.site0 = 0;  // (nothing of a block stays behind for the next run's stages)
        ctx->pend.pij = nullptr;
        if (gs != GDCA_OK) return gs;
        ldv[k] = ctx->ld.val[0];
        lds[k] = ctx->ld.src[0];
        if (k != 0) {
            bool tfail = false;
            ms_marg += elapsed(ctx, f == 0 ? T_TALLY_END : T_WEIGHTS, T_END, &tfail);
            if (f == 0) {
                ms_theta = sf.ms_theta;
                ms_weights = sf.ms_weights;
            }
            if (info) {
                info[k == 1 ? GDCA_LOGODDS_LOGDET_A : GDCA_LOGODDS_LOGDET_B] = ldv[k];
                info[k == 1 ? GDCA_LOGODDS_REFINED_A : GDCA_LOGODDS_REFINED_B] = (double)sf.refined;
            }
        }
    }
    st->ms_theta = ms_theta;
    st->ms_weights = ms_weights;
    for (int k = 0; k < 3; ++k) {
        ctx->ld.val[k] = ldv[k];
        ctx->ld.src[k] = lds[k];
    }
    ctx->ld.count = 3;
    if (info) {
        info[GDCA_LOGODDS_LOGDET] = ldv[0];
        info[GDCA_LOGODDS_INFORMATION] = ctx->pend.target.lo.I;
        info[GDCA_LOGODDS_MS_MARGINALS] = ms_marg;
    }
    return GDCA_OK;
}

gdca_status gdca_run_pair_logodds_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                      const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, double *L_dev, double *EmA_dev,
                                      double *EmB_dev, double *info, gdca_stats *st)
{
    CHK(check_run_pair(ctx, Z_dev, N, M, q, p, split, XA_dev, KA, XB_dev, KB, GDCA_PAIR_ENERGY, L_dev));
    return run_logodds(ctx, Z_dev, N, M, q, p, pair_target(Z_dev, N, M, split, XA_dev, KA, XB_dev, KB, GDCA_PAIR_ENERGY, L_dev), EmA_dev, EmB_dev, info,
                       st);
}

gdca_status gdca_run_partner_logodds_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                         const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, const void *offA, const void *offB,
                                         int32_t S, double *L_dev, int32_t *match_dev, double *gap_dev, double *info, gdca_stats *st)
{
    const int ka = XA_dev ? KA : M, kb = XB_dev ? KB : M;
    CHK(check_run_partner(ctx, Z_dev, N, M, q, p, split, ka, kb, offA, offB, GDCA_PAIR_ENERGY, match_dev));
    CHK(check_params(ctx, p));
    pair_blocks blk;
    std::vector<long long> first;
    CHK(species_blocks(ctx, offA, offB, S, ka, kb, (N - split) * (q - 1), true, &blk, first));
    if (!L_dev) {
        CHK(ensure(ctx, ctx->PBE, (size_t)blk.total * sizeof(double)));
        L_dev = (double *)ctx->PBE.p;
    }
    return run_logodds(ctx, Z_dev, N, M, q, p,
                       partner_target(pair_target(Z_dev, N, M, split, XA_dev, KA, XB_dev, KB, GDCA_PAIR_ENERGY, L_dev), blk, match_dev, gap_dev),
                       nullptr, nullptr, info, st);
}

// ---- iterative partner matching: the selection, the concatenation and the loop (k_ipa.hip) ----
// the selection enqueued: sel_dev and the counts record (ctx->IPAcnt)
static gdca_status select_stage(gdca_ctx *ctx, const int32_t *match_dev, const double *gap_dev, int KA, int n_take, int32_t *sel_dev)
{
    CHK(ensure(ctx, ctx->IPAws, gdca_ipa_select_ws_bytes(KA)));
    CHK(ensure(ctx, ctx->IPAcnt, sizeof(gdca_ipa_counts)));
    gdca_launch_ipa_select(ctx->stream, match_dev, gap_dev, KA, n_take, ctx->IPAws.p, sel_dev, (gdca_ipa_counts *)ctx->IPAcnt.p);
    return check_launch(ctx, "selection");
}

// the counts record on the host (one copy of a few scalars, one synchronisation)
static gdca_status fetch_counts(gdca_ctx *ctx, gdca_ipa_counts *h)
{
    HIPCHK(hipMemcpyAsync(h, ctx->IPAcnt.p, sizeof(*h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GDCA_OK;
}

static gdca_status check_select_confident(gdca_ctx *ctx, const void *match, const void *gap, int KA, const void *sel)
{
    if (!ctx) return GDCA_EINVAL;
    if (!match || !gap || !sel) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (KA < 1) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    return GDCA_OK;
}

gdca_status gdca_select_confident_dev(gdca_ctx *ctx, const int32_t *match_dev, const double *gap_dev, int32_t KA, int32_t n_take, int32_t *sel_dev,
                                      int32_t *n_sel)
{
    CHK(check_select_confident(ctx, match_dev, gap_dev, KA, sel_dev));
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    CHK(select_stage(ctx, match_dev, gap_dev, KA, n_take, sel_dev));
    gdca_ipa_counts h;
    CHK(fetch_counts(ctx, &h));
    if (n_sel) *n_sel = h.n_sel;
    return GDCA_OK;
}

// the argument checks of the two concatenation entry points (nothing has run when one fails)
static gdca_status validate_concat(gdca_ctx *ctx, const void *XA, int KA, const void *XB, int KB, int N, int split, const void *selA,
                                   const void *selB, int n_sel, const void *Z, long long col0)
{
    if (!ctx) return GDCA_EINVAL;
    if (N < 2 || split < 1 || split > N - 1) return fail(ctx, GDCA_EINVAL, "invalid split (must be between 1 and N - 1)");
    if (KA < 1 || KB < 1 || n_sel < 0 || col0 < 0 || col0 + n_sel > INT32_MAX) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    if (!XA || !XB || !Z || (n_sel > 0 && (!selA || !selB))) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_concat_pairs_dev(gdca_ctx *ctx, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, int32_t N, int32_t split,
                                  const int32_t *selA_dev, const int32_t *selB_dev, int32_t n_sel, int8_t *Z_dev, int32_t col0)
{
    CHK(validate_concat(ctx, XA_dev, KA, XB_dev, KB, N, split, selA_dev, selB_dev, n_sel, Z_dev, col0));
    CHK(begin(ctx));
    gdca_launch_ipa_concat(ctx->stream, XA_dev, KA, XB_dev, KB, N, split, selA_dev, selB_dev, nullptr, n_sel, Z_dev, (size_t)col0,
                           (gdca_dev_scalars *)ctx->sc.p);
    CHK(check_launch(ctx, "concatenation"));
    CHK(fetch_scalars(ctx));
    if (ctx->sc_host->bad_symbol & GDCA_BAD_INDEX) return fail(ctx, GDCA_EINVAL, "a selected index is outside its pool");
    return GDCA_OK;
}

// What gdca_run_partner_ipa(_dev) checks on the host before anything runs, and what the checks leave behind: the species of every a,
// and the seed as pairs in ascending a.
struct ipa_plan {
    std::vector<int32_t> spA, seedA, seedB;
};

static gdca_status ipa_check(gdca_ctx *ctx, int32_t KA, int32_t KB, const void *offA_, const void *offB_, int32_t S, int32_t N, int32_t q,
                             int32_t split, int32_t what, const gdca_params *p, int32_t Mfix, const int32_t *seedA, const int32_t *seedB,
                             int32_t n_seed, int32_t n_inc, int32_t max_rounds, const void *XA, const void *XB, const void *Zfix, const void *match,
                             ipa_plan *plan)
{
    if (!ctx) return GDCA_EINVAL;
    if (Mfix < 0 || n_seed < 0 || (long long)Mfix + n_seed < 1) return fail(ctx, GDCA_EINVAL, "no training pairs: Zfix and the seed are both empty");
    if (n_inc < 1 || max_rounds < 1) return fail(ctx, GDCA_EINVAL, "n_inc and max_rounds must be at least 1");
    CHK(validate_pair(ctx, N, q, split, KA, KB, what));
    if ((long long)Mfix + KA > INT32_MAX || (long long)Mfix + n_seed > INT32_MAX) return fail(ctx, GDCA_EINVAL, "invalid alignment size");
    if (!offA_ || !offB_ || !p || (n_seed > 0 && (!seedA || !seedB))) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(check_params(ctx, p));
    const int32_t *offA = (const int32_t *)offA_, *offB = (const int32_t *)offB_;
    int kmax = 0;
    if (blocks_length(offA, offB, S, &kmax) < 0 || offA[S] != KA || offB[S] != KB)
        return fail(ctx, GDCA_EINVAL, "invalid species offsets (S >= 1; from 0, non-decreasing, up to the number of sequences)");
    if (kmax > GDCA_ASSIGN_MAX) return fail(ctx, GDCA_EINVAL, "a species has more than GDCA_ASSIGN_MAX sequences on one side");
    plan->spA.assign((size_t)KA, 0);
    std::vector<int32_t> spB((size_t)KB, 0);
    for (int s = 0; s < S; ++s) {
        std::fill(plan->spA.begin() + offA[s], plan->spA.begin() + offA[s + 1], s);
        std::fill(spB.begin() + offB[s], spB.begin() + offB[s + 1], s);
    }
    std::vector<char> usedA((size_t)KA, 0), usedB((size_t)KB, 0);
    std::vector<std::pair<int32_t, int32_t>> seed;
    for (int t = 0; t < n_seed; ++t) {
        const int32_t a = seedA[t], b = seedB[t];
        if (a < 0 || a >= KA || b < 0 || b >= KB) return fail(ctx, GDCA_EINVAL, "a seed index is outside its pool");
        if (plan->spA[(size_t)a] != spB[(size_t)b]) return fail(ctx, GDCA_EINVAL, "a seed pair joins two species");
        if (usedA[(size_t)a] || usedB[(size_t)b]) return fail(ctx, GDCA_EINVAL, "a sequence appears twice in the seed");
        usedA[(size_t)a] = usedB[(size_t)b] = 1;
        seed.emplace_back(a, b);
    }
    std::sort(seed.begin(), seed.end());
    for (const auto &ab : seed) {
        plan->seedA.push_back(ab.first);
        plan->seedB.push_back(ab.second);
    }
    if (!XA || !XB || !match || (Mfix > 0 && !Zfix)) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_run_partner_ipa_dev(gdca_ctx *ctx, const int8_t *XA_dev, int32_t KA, const int8_t *XB_dev, int32_t KB, const void *offA,
                                     const void *offB, int32_t S, int32_t N, int32_t q, int32_t split, int32_t what, const gdca_params *p,
                                     const int8_t *Zfix_dev, int32_t Mfix, const int32_t *seedA, const int32_t *seedB, int32_t n_seed,
                                     int32_t n_inc, int32_t max_rounds, int32_t *match_dev, double *gap_dev, int32_t *match_trace_dev,
                                     double *gap_trace_dev, double *rounds_out, int32_t *rounds_run, gdca_stats *st)
{
    ipa_plan plan;
    CHK(ipa_check(ctx, KA, KB, offA, offB, S, N, q, split, what, p, Mfix, seedA, seedB, n_seed, n_inc, max_rounds, XA_dev, XB_dev, Zfix_dev, match_dev,
                  &plan));
    CHK(not_pending(ctx));
    if (rounds_run) *rounds_run = 0;
    hipStream_t s = ctx->stream;
    // ---- once per call: the species table and the gather's work list, the species of every a, the packed pools and their symbol check ----
    pair_blocks blk;
    std::vector<long long> first;
    CHK(species_blocks(ctx, offA, offB, S, KA, KB, (N - split) * (q - 1), true, &blk, first));
    const size_t ni = (size_t)KA * sizeof(int32_t), ng = (size_t)KA * sizeof(double);
    CHK(ensure(ctx, ctx->IPAsp, ni));
    CHK(ensure(ctx, ctx->IPAsel, 2 * ni));
    CHK(ensure(ctx, ctx->IPAm, ni));
    CHK(ensure(ctx, ctx->IPAg, ng));
    CHK(ensure(ctx, ctx->IPAprev, ni));
    CHK(ensure(ctx, ctx->IPAZ, (size_t)N * ((size_t)Mfix + (size_t)KA)));
    CHK(ensure(ctx, ctx->PBE, (size_t)blk.total * sizeof(double)));
    int32_t *sel = (int32_t *)ctx->IPAsel.p, *selB = sel + KA, *m_dev = (int32_t *)ctx->IPAm.p, *prev = (int32_t *)ctx->IPAprev.p;
    double *g_dev = (double *)ctx->IPAg.p, *E_dev = (double *)ctx->PBE.p;
    int8_t *Z = (int8_t *)ctx->IPAZ.p;
    HIPCHK(hipMemcpyAsync(ctx->IPAsp.p, plan.spA.data(), ni, hipMemcpyHostToDevice, s));
    if (n_seed > 0) {
        HIPCHK(hipMemcpyAsync(sel, plan.seedA.data(), (size_t)n_seed * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(selB, plan.seedB.data(), (size_t)n_seed * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    CHK(begin(ctx));
    CHK(pair_pack(ctx, N, q, split, XA_dev, (size_t)split, KA, XB_dev, (size_t)(N - split), KB, what));
    CHK(sequences_checked(ctx));  // (a synchronisation: the host arrays above have been read as well)
    // ---- the first training alignment: Zfix once, the seed behind it ----
    if (Mfix > 0) HIPCHK(hipMemcpyAsync(Z, Zfix_dev, (size_t)N * Mfix, hipMemcpyDeviceToDevice, s));
    gdca_launch_ipa_concat(s, XA_dev, KA, XB_dev, KB, N, split, sel, selB, nullptr, n_seed, Z, (size_t)Mfix, (gdca_dev_scalars *)ctx->sc.p);
    CHK(check_launch(ctx, "concatenation"));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const bool timed = ctx->timing && rounds_out;
    if (timed && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) {
        if (ev0) (void)hipEventDestroy(ev0);
        return fail(ctx, GDCA_EHIP, "hipEventCreate");
    }
    gdca_status rs = GDCA_OK;
    int M = Mfix + n_seed, sel_before = -1, cand_before = -2;
    for (int r = 1; r <= max_rounds; ++r) {
        // ---- fit and match: the fused partner match's own code on Z_r, the pools as packed above ----
        score_target t = partner_target(pair_target(Z, N, M, split, XA_dev, KA, XB_dev, KB, what, E_dev), blk, m_dev, g_dev);
        t.packed = true;
        gdca_stats fit;
        rs = run_target(ctx, Z, N, M, q, p, t, &fit);
        if (st) *st = fit;
        if (rs != GDCA_OK) break;
        // ---- the round is complete: its figures, its results where the caller wants them, the selection ----
        gdca_status gs = GDCA_OK;
        auto step = [&](hipError_t e) {
            if (e != hipSuccess && gs == GDCA_OK) gs = fail(ctx, GDCA_EHIP, "iterative partner matching: %s%s", hipGetErrorString(e), "");
        };
        if (timed) step(hipEventRecord(ev0, s));
        gs = gs != GDCA_OK ? gs : ensure(ctx, ctx->IPAcnt, sizeof(gdca_ipa_counts));
        if (gs == GDCA_OK) {
            gdca_launch_ipa_round(s, E_dev, blk.eoff, blk.offA, blk.offB, (const int32_t *)ctx->IPAsp.p, m_dev, r > 1 ? prev : nullptr, KA,
                                  (gdca_ipa_counts *)ctx->IPAcnt.p);
            gs = check_launch(ctx, "round figures");
        }
        if (gs == GDCA_OK) {  // (behind the figures: they read the match of the round before)
            gdca_launch_ipa_publish(s, m_dev, g_dev, KA, prev, match_dev, gap_dev, match_trace_dev ? match_trace_dev + (size_t)(r - 1) * KA : nullptr,
                                    gap_trace_dev ? gap_trace_dev + (size_t)(r - 1) * KA : nullptr);
            gs = check_launch(ctx, "round results");
        }
        const int n_take = (int)std::min<long long>((long long)r * n_inc, KA);
        if (gs == GDCA_OK) gs = select_stage(ctx, m_dev, g_dev, KA, n_take, sel);
        if (timed) step(hipEventRecord(ev1, s));
        gdca_ipa_counts h{};
        if (gs == GDCA_OK) gs = fetch_counts(ctx, &h);
        if (gs != GDCA_OK) {
            rs = gs;
            break;
        }
        if (rounds_out) {
            double *row = rounds_out + (size_t)(r - 1) * GDCA_IPA_FIELDS;
            float ms = 0.0f;
            if (timed) step(hipEventElapsedTime(&ms, ev0, ev1));
            row[GDCA_IPA_M_TRAIN] = (double)M;
            row[GDCA_IPA_CANDIDATES] = (double)h.ncand;
            row[GDCA_IPA_N_SEL] = (double)h.n_sel;
            row[GDCA_IPA_N_CHANGED] = (double)h.n_changed;
            row[GDCA_IPA_MEFF] = fit.Meff;
            row[GDCA_IPA_THETA] = fit.theta;
            row[GDCA_IPA_LOGDET] = ctx->ld.count > 0 ? ctx->ld.val[0] : (double)NAN;
            row[GDCA_IPA_COST] = h.cost;
            row[GDCA_IPA_MS_FIT] = fit.ms_total - fit.ms_score;
            row[GDCA_IPA_MS_MATCH] = fit.ms_score;
            row[GDCA_IPA_MS_SELECT] = (double)ms;
            row[GDCA_IPA_RESERVED] = 0.0;
        }
        if (rounds_run) *rounds_run = r;
        // ---- the stop rule, else the next training alignment: Zfix stays, the selected pairs behind it in ascending a ----
        if (r == max_rounds || (r >= 2 && sel_before == cand_before) || Mfix + h.n_sel < 1) break;
        gdca_launch_ipa_concat(s, XA_dev, KA, XB_dev, KB, N, split, sel, nullptr, m_dev, h.n_sel, Z, (size_t)Mfix, (gdca_dev_scalars *)ctx->sc.p);
        rs = check_launch(ctx, "concatenation");
        if (rs != GDCA_OK) break;
        M = Mfix + h.n_sel;
        sel_before = h.n_sel;
        cand_before = h.ncand;
    }
    (void)hipStreamSynchronize(s);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rs;
}

// the argument checks the four mutation-scan entry points share (nothing has run when one fails); K as it will be used
static gdca_status validate_mutation(gdca_ctx *ctx, int N, int q, long long K, int what)
{
    CHK(validate(ctx, N, 1, q));
    // (the grids round K up to whole workgroups of 256 sequences in 32-bit arithmetic)
    if (K < 1 || K > INT32_MAX - 256) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    if (what != GDCA_MUT_DELTA && what != GDCA_MUT_POTENTIAL) return fail(ctx, GDCA_EINVAL, "invalid value of `what`");
    return GDCA_OK;
}

static gdca_status check_mutation_scan(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *X, int K, int what, const void *D)
{
    CHK(validate_mutation(ctx, N, q, K, what));
    if (!mJ || !Pi || !X || !D) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

static gdca_status check_run_mutation_scan(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, const void *X, int K, int what,
                                           const void *D)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_mutation(ctx, N, q, X ? K : M, what));
    if (!Z || !D || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_mutation_scan_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                   int32_t K, int32_t what, double *D_dev)
{
    CHK(check_mutation_scan(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, what, D_dev));
    CHK(begin(ctx));
    CHK(mutation_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), X_dev, K, what, D_dev));
    return sequences_checked(ctx);
}

gdca_status gdca_run_mutation_scan_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                       const int8_t *X_dev, int32_t K, int32_t what, double *D_dev, gdca_stats *st)
{
    CHK(check_run_mutation_scan(ctx, Z_dev, N, M, q, p, X_dev, K, what, D_dev));
    return run_target(ctx, Z_dev, N, M, q, p, mutation_target(Z_dev, M, X_dev, K, what, D_dev), st);
}

// the argument checks the double-mutant entry points share (nothing has run when one fails)
static gdca_status validate_double(gdca_ctx *ctx, int N, int q, long long K)
{
    CHK(validate(ctx, N, 1, q));
    if (N < 2) return fail(ctx, GDCA_EINVAL, "a double mutant needs two sites");
    if (K < 1 || K > INT32_MAX - 256) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    const long long nT = (N + 3) / 4;
    if ((K + 63) / 64 * (nT * (nT + 1) / 2) > GDCA_EPI_MAX_GROUPS) return fail(ctx, GDCA_EINVAL, "N^2 K is too large for one scan");
    return GDCA_OK;
}

// the scan's and the listed form's: `a` and `b` are the model, mJ and Pi (M: 1), or -- a fused form -- the alignment of M sequences and
// its parameters
static gdca_status check_double_scan(gdca_ctx *ctx, const void *a, const void *b, int N, int M, int q, const void *X, int K, const void *Emin,
                                     const void *code, const void *epi)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_double(ctx, N, q, K));
    if (!a || !b || !X) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (!Emin && !code && !epi) return fail(ctx, GDCA_EINVAL, "no output requested");
    return GDCA_OK;
}

static gdca_status check_double_list(gdca_ctx *ctx, const void *a, const void *b, int N, int M, int q, const void *X, int K, const void *muts, int L,
                                     const void *out)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_double(ctx, N, q, K));
    if (L < 1) return fail(ctx, GDCA_EINVAL, "invalid number of double mutants");
    if (!a || !b || !X || !muts || !out) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_double_mutant_scan_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                        int32_t K, double *Emin_dev, int32_t *code_dev, double *epi_dev)
{
    CHK(check_double_scan(ctx, mJ_dev, Pi_dev, N, 1, q, X_dev, K, Emin_dev, code_dev, epi_dev));
    CHK(begin(ctx));
    CHK(double_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), X_dev, K, Emin_dev, code_dev, epi_dev, nullptr, 0, nullptr));
    return sequences_checked(ctx);
}

gdca_status gdca_double_mutants_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                    int32_t K, const void *muts_dev, int32_t L, double *out_dev)
{
    CHK(check_double_list(ctx, mJ_dev, Pi_dev, N, 1, q, X_dev, K, muts_dev, L, out_dev));
    CHK(begin(ctx));
    CHK(double_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), X_dev, K, nullptr, nullptr, nullptr, (const int32_t *)muts_dev, L, out_dev));
    return sequences_checked(ctx);
}

gdca_status gdca_run_double_mutant_scan_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                            const int8_t *X_dev, int32_t K, double *Emin_dev, int32_t *code_dev, double *epi_dev, gdca_stats *st)
{
    CHK(check_double_scan(ctx, Z_dev, p, N, M, q, X_dev, K, Emin_dev, code_dev, epi_dev));
    return run_target(ctx, Z_dev, N, M, q, p, double_scan_target(X_dev, K, Emin_dev, code_dev, epi_dev), st);
}

gdca_status gdca_run_double_mutants_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                        const int8_t *X_dev, int32_t K, const void *muts_dev, int32_t L, double *out_dev, gdca_stats *st)
{
    CHK(check_double_list(ctx, Z_dev, p, N, M, q, X_dev, K, muts_dev, L, out_dev));
    return run_target(ctx, Z_dev, N, M, q, p, double_list_target(X_dev, K, (const int32_t *)muts_dev, L, out_dev), st);
}

// the argument checks the four greedy-walk entry points share (nothing has run when one fails); K as it will be used
static gdca_status validate_walk(gdca_ctx *ctx, int N, int q, long long K, int flags, double min_gain, int max_steps, const void *Xout,
                                 const void *steps)
{
    CHK(validate(ctx, N, 1, q));
    if (K < 1 || K > INT32_MAX - 256) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    if (max_steps < 1 || max_steps > GDCA_WALK_MAX_STEPS) return fail(ctx, GDCA_EINVAL, "invalid max_steps");
    if (!(min_gain >= 0.0)) return fail(ctx, GDCA_EINVAL, "invalid min_gain");
    if (flags & ~(GDCA_WALK_GAP_TARGET | GDCA_WALK_FILL_GAPS)) return fail(ctx, GDCA_EINVAL, "invalid flags");
    if (!Xout || !steps) return fail(ctx, GDCA_EINVAL, "null pointer");
    bool in_lds = false;
    CHK(walk_placement(ctx, N, q, &in_lds));
    return GDCA_OK;
}

static gdca_status check_greedy_walk(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *X, int K, int flags, double min_gain,
                                     int max_steps, const void *Xout, const void *steps)
{
    CHK(validate_walk(ctx, N, q, K, flags, min_gain, max_steps, Xout, steps));
    if (!mJ || !Pi || !X) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

static gdca_status check_run_greedy_walk(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, const void *X, int K, int flags,
                                         double min_gain, int max_steps, const void *Xout, const void *steps)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_walk(ctx, N, q, X ? K : M, flags, min_gain, max_steps, Xout, steps));
    if (!Z || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_greedy_walk_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev,
                                 int32_t K, const int8_t *mask_dev, int32_t flags, double min_gain, int32_t max_steps, int8_t *Xout_dev,
                                 int32_t *steps_dev, double *dE_sum_dev, int32_t *path_dev, double *dE_path_dev, double *V_dev)
{
    CHK(check_greedy_walk(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, flags, min_gain, max_steps, Xout_dev, steps_dev));
    CHK(begin(ctx));
    const walk_request w{mask_dev, flags, max_steps, min_gain, Xout_dev, steps_dev, dE_sum_dev, path_dev, dE_path_dev, V_dev};
    CHK(walk_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), X_dev, K, w));
    return sequences_checked(ctx);
}

gdca_status gdca_run_greedy_walk_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                     const int8_t *X_dev, int32_t K, const int8_t *mask_dev, int32_t flags, double min_gain,
                                     int32_t max_steps, int8_t *Xout_dev, int32_t *steps_dev, double *dE_sum_dev, int32_t *path_dev,
                                     double *dE_path_dev, double *V_dev, gdca_stats *st)
{
    CHK(check_run_greedy_walk(ctx, Z_dev, N, M, q, p, X_dev, K, flags, min_gain, max_steps, Xout_dev, steps_dev));
    const walk_request w{mask_dev, flags, max_steps, min_gain, Xout_dev, steps_dev, dE_sum_dev, path_dev, dE_path_dev, V_dev};
    return run_target(ctx, Z_dev, N, M, q, p, walk_target(Z_dev, M, X_dev, K, w), st);
}

// the argument checks the four Metropolis entry points share (nothing has run when one fails); K as it will be used
static gdca_status validate_sample(gdca_ctx *ctx, int N, int q, long long K, int flags, double beta, int burn, int stride, int n_samples,
                                   const void *Xs, const void *accepted)
{
    CHK(validate(ctx, N, 1, q));
    if (K < 1 || K > INT32_MAX - 256) return fail(ctx, GDCA_EINVAL, "invalid number of sequences");
    if (flags & ~GDCA_SAMPLE_GAPS) return fail(ctx, GDCA_EINVAL, "invalid flags");
    if ((flags & GDCA_SAMPLE_GAPS ? q : q - 1) < 2) return fail(ctx, GDCA_EINVAL, "fewer than two target symbols");
    if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(ctx, GDCA_EINVAL, "invalid beta");
    if (burn < 0 || stride < 1 || n_samples < 1 || (long long)burn + (long long)n_samples * stride > INT32_MAX)
        return fail(ctx, GDCA_EINVAL, "invalid burn, stride or n_samples");
    if (!Xs || !accepted) return fail(ctx, GDCA_EINVAL, "null pointer");
    bool in_lds = false;
    CHK(walk_placement(ctx, N, q, &in_lds));
    if (N > GDCA_SAMPLE_MAX_SITES) return fail(ctx, GDCA_EINVAL, "N is larger than GDCA_SAMPLE_MAX_SITES");
    return GDCA_OK;
}

static gdca_status check_sample(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *X, int K, int flags, double beta,
                                int burn, int stride, int n_samples, const void *Xs, const void *accepted)
{
    CHK(validate_sample(ctx, N, q, K, flags, beta, burn, stride, n_samples, Xs, accepted));
    if (!mJ || !Pi || !X) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

static gdca_status check_run_sample(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, const void *X, int K, int flags,
                                    double beta, int burn, int stride, int n_samples, const void *Xs, const void *accepted)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_sample(ctx, N, q, X ? K : M, flags, beta, burn, stride, n_samples, Xs, accepted));
    if (!Z || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_sample_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *X_dev, int32_t K,
                            const int8_t *mask_dev, int32_t flags, double beta, uint64_t seed, uint64_t stream0, int32_t burn,
                            int32_t stride, int32_t n_samples, int8_t *Xs_dev, double *dE_s_dev, int32_t *accepted_dev, double *thr_dev,
                            int32_t *moves_dev, double *V_dev)
{
    CHK(check_sample(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, flags, beta, burn, stride, n_samples, Xs_dev, accepted_dev));
    CHK(begin(ctx));
    const sample_request r{{{mask_dev, flags, seed, stream0, burn, stride, n_samples, thr_dev, moves_dev}, beta, Xs_dev, dE_s_dev, accepted_dev},
                           V_dev};
    CHK(sample_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), X_dev, K, r));
    return sequences_checked(ctx);
}

gdca_status gdca_run_sample_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                const int8_t *X_dev, int32_t K, const int8_t *mask_dev, int32_t flags, double beta, uint64_t seed,
                                uint64_t stream0, int32_t burn, int32_t stride, int32_t n_samples, int8_t *Xs_dev, double *dE_s_dev,
                                int32_t *accepted_dev, double *thr_dev, int32_t *moves_dev, double *V_dev, gdca_stats *st)
{
    CHK(check_run_sample(ctx, Z_dev, N, M, q, p, X_dev, K, flags, beta, burn, stride, n_samples, Xs_dev, accepted_dev));
    const sample_request r{{{mask_dev, flags, seed, stream0, burn, stride, n_samples, thr_dev, moves_dev}, beta, Xs_dev, dE_s_dev, accepted_dev},
                           V_dev};
    return run_target(ctx, Z_dev, N, M, q, p, sample_target(Z_dev, M, X_dev, K, r), st);
}

// the argument checks of the two log-partition entry points (nothing has run when one fails)
static gdca_status check_log_partition(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *x, const void *mask, int flags,
                                       const double *betas, int L, int sweep, int K, const void *out4, const void *logw)
{
    if (L < 1 || sweep < 1) return fail(ctx, GDCA_EINVAL, "invalid L or sweep: each must be at least 1");
    if ((long long)L * (long long)sweep > INT32_MAX) return fail(ctx, GDCA_EINVAL, "L * sweep is larger than INT32_MAX");
    if (!betas || !out4 || !logw) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(validate_sample(ctx, N, q, K, flags, 0.0, 0, sweep, L, out4, logw));
    if (betas[0] != 0.0) return fail(ctx, GDCA_EINVAL, "invalid betas: betas[0] must be 0 (the base distribution is the uniform one)");
    for (int l = 0; l <= L; ++l)
        if (!(betas[l] >= 0.0) || !std::isfinite(betas[l])) return fail(ctx, GDCA_EINVAL, "invalid betas: every beta must be finite and >= 0");
    if (!mJ || !Pi) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (!x && mask) return fail(ctx, GDCA_EINVAL, "a mask needs a template x");
    return GDCA_OK;
}

gdca_status gdca_log_partition_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *x_dev,
                                   const int8_t *mask_dev, int32_t flags, const double *betas, int32_t L, int32_t sweep, int32_t K,
                                   uint64_t seed, uint64_t stream0, double *out4_dev, double *logw_dev, double *E_end_dev, int8_t *X0_dev,
                                   int8_t *Xout_dev, int32_t *accepted_dev, double *thr_dev, int32_t *moves_dev)
{
    CHK(check_log_partition(ctx, mJ_dev, Pi_dev, N, q, x_dev, mask_dev, flags, betas, L, sweep, K, out4_dev, logw_dev));
    CHK(begin(ctx));
    const gdca_ais_plan plan{{mask_dev, flags, seed, stream0, 0, sweep, L, thr_dev, moves_dev}, L, sweep, nullptr, out4_dev, logw_dev, E_end_dev,
                             X0_dev, Xout_dev, accepted_dev};
    CHK(ais_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), x_dev, K, betas, plan));
    return sequences_checked(ctx);
}

// the argument checks the four replica-exchange entry points share (nothing has run when one fails); K chains as they will be used
static gdca_status validate_temper(gdca_ctx *ctx, int N, int q, long long K, int R, const double *betas, int flags, int swap_every, int burn,
                                   int stride, int n_samples, const void *Xs, const void *accepted, const void *swaps, const void *Xr_out,
                                   const void *slot_out)
{
    if (R < 1 || R > GDCA_TEMPER_MAX) return fail(ctx, GDCA_EINVAL, "invalid number of replicas");
    if (!betas) return fail(ctx, GDCA_EINVAL, "null pointer");
    for (int r = 0; r < R; ++r) CHK(validate_sample(ctx, N, q, K < 1 ? K : K * R, flags, betas[r], burn, stride, n_samples, Xs, accepted));
    if (!swaps || !Xr_out || !slot_out) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (swap_every < 1 || burn % swap_every != 0 || stride % swap_every != 0)
        return fail(ctx, GDCA_EINVAL, "invalid swap_every: it must be at least 1 and divide burn and stride");
    return GDCA_OK;
}

static temper_request temper_request_of(int R, const double *betas, const int8_t *mask, int flags, uint64_t seed, uint64_t stream0, int swap_every,
                                        int burn, int stride, int n_samples, const int32_t *slot0, int8_t *Xs, double *E_s, int32_t *accepted,
                                        int32_t *swaps, int8_t *Xr_out, int32_t *slot_out, double *thr, int32_t *moves, double *swap_thr,
                                        int32_t *slot_path, bool fused)
{
    temper_request r{};
    r.plan.chain = gdca_chain_plan{mask, flags, seed, stream0, burn, stride, n_samples, thr, moves};
    r.plan.R = R, r.plan.swap_every = swap_every;
    for (int i = 0; i < R; ++i) r.plan.betas[i] = betas[i];
    r.plan.slot0 = slot0, r.plan.Xs = Xs, r.plan.E_s = E_s, r.plan.accepted = accepted, r.plan.swaps = swaps, r.plan.Xr_out = Xr_out;
    r.plan.slot_out = slot_out, r.plan.swap_thr = swap_thr, r.plan.slot_path = slot_path;
    r.fused = fused;
    return r;
}

static gdca_status check_sample_tempered(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *Xr, int K, int R,
                                         const double *betas, int flags, int swap_every, int burn, int stride, int n_samples, const void *Xs,
                                         const void *accepted, const void *swaps, const void *Xr_out, const void *slot_out)
{
    CHK(validate_temper(ctx, N, q, K, R, betas, flags, swap_every, burn, stride, n_samples, Xs, accepted, swaps, Xr_out, slot_out));
    if (!mJ || !Pi || !Xr) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

static gdca_status check_run_sample_tempered(gdca_ctx *ctx, const void *Z, int N, int M, int q, const void *p, const void *X, int K, int R,
                                             const double *betas, int flags, int swap_every, int burn, int stride, int n_samples,
                                             const void *Xs, const void *accepted, const void *swaps, const void *Xr_out,
                                             const void *slot_out)
{
    CHK(validate(ctx, N, M, q));
    CHK(validate_temper(ctx, N, q, X ? K : M, R, betas, flags, swap_every, burn, stride, n_samples, Xs, accepted, swaps, Xr_out, slot_out));
    if (!Z || !p) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

gdca_status gdca_sample_tempered_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, const int8_t *Xr_dev,
                                     const int32_t *slot0_dev, int32_t K, int32_t R, const double *betas, const int8_t *mask_dev,
                                     int32_t flags, uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride,
                                     int32_t n_samples, int8_t *Xs_dev, double *E_s_dev, int32_t *accepted_dev, int32_t *swaps_dev,
                                     int8_t *Xr_out_dev, int32_t *slot_out_dev, double *thr_dev, int32_t *moves_dev, double *swap_thr_dev,
                                     int32_t *slot_path_dev)
{
    CHK(check_sample_tempered(ctx, mJ_dev, Pi_dev, N, q, Xr_dev, K, R, betas, flags, swap_every, burn, stride, n_samples, Xs_dev, accepted_dev,
                              swaps_dev, Xr_out_dev, slot_out_dev));
    CHK(begin(ctx));
    const temper_request r = temper_request_of(R, betas, mask_dev, flags, seed, stream0, swap_every, burn, stride, n_samples, slot0_dev, Xs_dev,
                                               E_s_dev, accepted_dev, swaps_dev, Xr_out_dev, slot_out_dev, thr_dev, moves_dev, swap_thr_dev,
                                               slot_path_dev, false);
    CHK(temper_stage(ctx, operator_model(mJ_dev, Pi_dev, N, q), Xr_dev, K, r));
    CHK(fetch_scalars(ctx));
    if (ctx->sc_host->bad_symbol & GDCA_BAD_SLOTS) return fail(ctx, GDCA_EINVAL, "a column of slot0 is not a permutation of 0 .. R - 1");
    return conclude(ctx, GDCA_ENDS_READOUT);
}

gdca_status gdca_run_sample_tempered_dev(gdca_ctx *ctx, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                         const int8_t *X_dev, int32_t K, int32_t R, const double *betas, const int8_t *mask_dev,
                                         int32_t flags, uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride,
                                         int32_t n_samples, int8_t *Xs_dev, double *E_s_dev, int32_t *accepted_dev, int32_t *swaps_dev,
                                         int8_t *Xr_out_dev, int32_t *slot_out_dev, double *thr_dev, int32_t *moves_dev,
                                         double *swap_thr_dev, int32_t *slot_path_dev, gdca_stats *st)
{
    CHK(check_run_sample_tempered(ctx, Z_dev, N, M, q, p, X_dev, K, R, betas, flags, swap_every, burn, stride, n_samples, Xs_dev, accepted_dev,
                                  swaps_dev, Xr_out_dev, slot_out_dev));
    const temper_request r = temper_request_of(R, betas, mask_dev, flags, seed, stream0, swap_every, burn, stride, n_samples, nullptr, Xs_dev,
                                               E_s_dev, accepted_dev, swaps_dev, Xr_out_dev, slot_out_dev, thr_dev, moves_dev, swap_thr_dev,
                                               slot_path_dev, true);
    return run_target(ctx, Z_dev, N, M, q, p, temper_target(Z_dev, M, X_dev, K, r), st);
}

// ---- Boltzmann-machine refinement (k_bm.hip; include/gdca.h): the warm start, the update, the read-out and the loop ----
static gdca_status check_potts(gdca_ctx *ctx, const void *mJ, const void *Pi, int N, int q, const void *W)
{
    CHK(validate(ctx, N, 1, q));
    if (!mJ || !Pi || !W) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (mJ == W) return fail(ctx, GDCA_EINVAL, "W may not alias mJ");
    return GDCA_OK;
}

static gdca_status check_bm_rates(gdca_ctx *ctx, double eta, double lambda)
{
    if (!(eta > 0.0) || !std::isfinite(eta)) return fail(ctx, GDCA_EINVAL, "invalid eta");
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(ctx, GDCA_EINVAL, "invalid lambda");
    return GDCA_OK;
}

static gdca_status check_bm_update(gdca_ctx *ctx, const void *W, const void *Pij_d, const void *Pij_m, int N, int q, double eta, double lambda)
{
    CHK(validate(ctx, N, 1, q));
    if (!W || !Pij_d || !Pij_m) return fail(ctx, GDCA_EINVAL, "null pointer");
    return check_bm_rates(ctx, eta, lambda);
}

static gdca_status check_bm_readout(gdca_ctx *ctx, const void *Pi_d, const void *Pij_d, const void *Pi_m, const void *Pij_m, int N, int q,
                                    const void *out)
{
    CHK(validate(ctx, N, 1, q));
    if (!Pi_d || !Pij_d || !Pi_m || !Pij_m || !out) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

// the loop's arguments: validate_sample's, the rates, the iteration range; nothing has run when one fails
static gdca_status check_bm_learn(gdca_ctx *ctx, const void *W, const void *Pi_d, const void *Pij_d, int N, int q, const void *X, int K,
                                  int flags, double beta, uint64_t iter0, int n_iter, int burn, int stride, int n_samples, double eta,
                                  double lambda, const void *trace)
{
    CHK(validate_sample(ctx, N, q, K, flags, beta, burn, stride, n_samples, W, W));  // (Xs and accepted are the loop's own)
    if (!W || !Pi_d || !Pij_d || !X || !trace) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(check_bm_rates(ctx, eta, lambda));
    if (n_iter < 1) return fail(ctx, GDCA_EINVAL, "invalid n_iter");
    if ((long long)K * n_samples > INT32_MAX) return fail(ctx, GDCA_EINVAL, "K n_samples is larger than INT32_MAX");
    // iteration t draws from the streams t K .. t K + K - 1
    if (((unsigned __int128)iter0 + (unsigned)n_iter) * (unsigned __int128)(unsigned)K > (unsigned __int128)UINT64_MAX)
        return fail(ctx, GDCA_EINVAL, "(iter0 + n_iter) K overflows the stream numbers");
    return GDCA_OK;
}

gdca_status gdca_potts_from_gaussian_dev(gdca_ctx *ctx, const double *mJ_dev, const double *Pi_dev, int32_t N, int32_t q, double *W_dev)
{
    CHK(check_potts(ctx, mJ_dev, Pi_dev, N, q, W_dev));
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    CHK(g_room(ctx, N * (q - 1)));
    g_launch(ctx, operator_model(mJ_dev, Pi_dev, N, q));
    gdca_launch_bm_from_gaussian(ctx->stream, mJ_dev, (const double *)ctx->gvec.p, N, q - 1, W_dev);
    return check_launch(ctx, "Potts warm start");
}

gdca_status gdca_bm_update_dev(gdca_ctx *ctx, double *W_dev, const double *Pi_d_dev, const double *Pij_d_dev, const double *Pi_m_dev,
                               const double *Pij_m_dev, int32_t N, int32_t q, double eta, double lambda)
{
    (void)Pi_d_dev, (void)Pi_m_dev;  // (the diagonal works through Pij alone)
    CHK(check_bm_update(ctx, W_dev, Pij_d_dev, Pij_m_dev, N, q, eta, lambda));
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    gdca_launch_bm_update(ctx->stream, W_dev, Pij_d_dev, Pij_m_dev, N, q - 1, eta, lambda);
    return check_launch(ctx, "Boltzmann-machine update");
}

static gdca_status bm_readout_stage(gdca_ctx *ctx, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int N, int q,
                                    double *out, bool zero3)
{
    CHK(ensure(ctx, ctx->BMred, gdca_bm_readout_bytes(N * (q - 1))));
    gdca_launch_bm_readout(ctx->stream, Pi_d, Pij_d, Pi_m, Pij_m, N, q - 1, (double *)ctx->BMred.p, out, zero3);
    return check_launch(ctx, "Boltzmann-machine read-out");
}

gdca_status gdca_bm_readout_dev(gdca_ctx *ctx, const double *Pi_d_dev, const double *Pij_d_dev, const double *Pi_m_dev,
                                const double *Pij_m_dev, int32_t N, int32_t q, double *out4_dev)
{
    CHK(check_bm_readout(ctx, Pi_d_dev, Pij_d_dev, Pi_m_dev, Pij_m_dev, N, q, out4_dev));
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    return bm_readout_stage(ctx, Pi_d_dev, Pij_d_dev, Pi_m_dev, Pij_m_dev, N, q, out4_dev, true);
}

// where the loop's arrays lie in ctx->BMws (each at a multiple of 256 bytes): the model's tallies Pij_m (n x n) and Pi_m (n), the zero
// Pi of the container (n), the unit weights (K n_samples), the chains' counts (K), the samples (N x n_samples x K; not where the caller
// gives Xs_last)
struct bm_plan {
    size_t pij, pi, zero, ones, acc, xs, bytes;
    bm_plan(int n, int N, int K, int S, bool own_xs)
    {
        size_t at = 0;
        auto take = [&](size_t b) {
            const size_t here = at;
            at += (b + 255) & ~(size_t)255;
            return here;
        };
        pij = take((size_t)n * n * sizeof(double));
        pi = take((size_t)n * sizeof(double));
        zero = take((size_t)n * sizeof(double));
        ones = take((size_t)K * S * sizeof(double));
        acc = take((size_t)K * sizeof(int32_t));
        xs = take(own_xs ? (size_t)N * S * K : 0);
        bytes = at;
    }
};

gdca_status gdca_bm_learn_dev(gdca_ctx *ctx, double *W_dev, const double *Pi_d_dev, const double *Pij_d_dev, int32_t N, int32_t q,
                              int8_t *X_dev, int32_t K, const int8_t *mask_dev, int32_t flags, double beta, uint64_t seed, uint64_t iter0,
                              int32_t n_iter, int32_t burn, int32_t stride, int32_t n_samples, double eta, double lambda, double *trace_dev,
                              int8_t *Xs_last_dev)
{
    CHK(check_bm_learn(ctx, W_dev, Pi_d_dev, Pij_d_dev, N, q, X_dev, K, flags, beta, iter0, n_iter, burn, stride, n_samples, eta, lambda,
                       trace_dev));
    CHK(begin(ctx));
    hipStream_t s = ctx->stream;
    const int sdim = q - 1, n = N * sdim, M = K * n_samples;
    const long long n_steps = (long long)burn + (long long)n_samples * stride;
    const bm_plan at(n, N, K, n_samples, Xs_last_dev == nullptr);
    CHK(ensure(ctx, ctx->BMws, at.bytes));
    CHK(ensure(ctx, ctx->Wfix, (size_t)M * sizeof(unsigned long long)));
    char *ws = (char *)ctx->BMws.p;
    double *Pij_m = (double *)(ws + at.pij), *Pi_m = (double *)(ws + at.pi), *zero = (double *)(ws + at.zero), *ones = (double *)(ws + at.ones);
    int32_t *accepted = (int32_t *)(ws + at.acc);
    int8_t *Xs = Xs_last_dev ? Xs_last_dev : (int8_t *)(ws + at.xs);
    gdca_dev_scalars *sc = (gdca_dev_scalars *)ctx->sc.p;
    // what does not change over the loop: the zero Pi, the unit weights in the tally's fixed point, Meff = K n_samples
    // (gdca_frequencies_dev's own calls, so the tallies are its bits)
    const double Meff = (double)M;
    gdca_launch_bm_fill(s, zero, (size_t)n, 0.0);
    gdca_launch_bm_fill(s, ones, (size_t)M, 1.0);
    HIPCHK(hipMemcpyAsync(&sc->Meff, &Meff, sizeof(double), hipMemcpyHostToDevice, s));
    gdca_launch_fix_weights(s, ones, M, gdca_fix_shift(M), (unsigned long long *)ctx->Wfix.p, sc);
    const gdca_model model = operator_model(W_dev, zero, N, q);
    for (int it = 0; it < n_iter; ++it) {
        const uint64_t t = iter0 + (uint64_t)it;
        const sample_request r{{{mask_dev, flags, seed, t * (uint64_t)K, burn, stride, n_samples, nullptr, nullptr}, beta, Xs, nullptr, accepted},
                               nullptr};
        CHK(sample_stage(ctx, model, X_dev, K, r));
        gdca_launch_bm_last_sample(s, Xs, N, K, n_samples, X_dev);
        CHK(tally_stage(ctx, Xs, N, M, q, &sc->Meff, 0.0, 0, Pi_m, Pij_m, (size_t)n));
        double *out = trace_dev + 4 * (size_t)it;
        CHK(bm_readout_stage(ctx, Pi_d_dev, Pij_d_dev, Pi_m, Pij_m, N, q, out, false));
        gdca_launch_bm_accept(s, accepted, K, n_steps, out + 3);
        gdca_launch_bm_update(s, W_dev, Pij_d_dev, Pij_m, N, sdim, eta, lambda);
        CHK(check_launch(ctx, "Boltzmann-machine iteration"));
    }
    return sequences_checked(ctx);  // (the one round trip of the call: the device's flags)
}

// ---- pseudo-likelihood fit (k_plm.hip; include/gdca.h): the conditionals, their tally, the two fused over slabs, the loop ----
// The sequences go through the mutation stage in SLABS of whole blocks of PLM_CHUNK, so the table [slab][N][q] stays bounded: 256 MB
// where PLM_SLAB does not say otherwise.  A block never straddles two slabs, so the order of every sum is the same whatever the slab.
struct plm_geometry {
    int chunk, slab;
    plm_geometry(const gdca_ctx *ctx, int N, int M, int q)
    {
        chunk = ctx->tune.plm_chunk > 0 ? ctx->tune.plm_chunk : GDCA_PLM_CHUNK_RULE;
        long long want = ctx->tune.plm_slab > 0 ? ctx->tune.plm_slab : std::max(1LL, (256LL << 20) / ((long long)N * q * 8));
        want = (want + chunk - 1) / chunk * chunk;
        slab = (int)std::min<long long>(want, ((long long)M + chunk - 1) / chunk * chunk);
    }
};

// where the arrays lie in ctx->PLMws (each at a multiple of 256 bytes): Q (n x n), S (n), the zero Pi of the container (n), nll_k (M),
// l_ki of a slab (slab N), and the loop's own conditional tallies Pij_c (n x n), Pi_c (n) and nll (1)
struct plm_plan {
    size_t q, s, zero, nllk, l, pij, pi, nll, bytes;
    plm_plan(int n, int N, int M, int slab, bool loop)
    {
        size_t at = 0;
        auto take = [&](size_t b) {
            const size_t here = at;
            at += (b + 255) & ~(size_t)255;
            return here;
        };
        q = take((size_t)n * n * sizeof(double));
        s = take((size_t)n * sizeof(double));
        zero = take((size_t)n * sizeof(double));
        nllk = take((size_t)M * sizeof(double));
        l = take((size_t)std::min(slab, M) * N * sizeof(double));
        pij = take(loop ? (size_t)n * n * sizeof(double) : 0);
        pi = take(loop ? (size_t)n * sizeof(double) : 0);
        nll = take(sizeof(double));
        bytes = at;
    }
};

static gdca_status check_plm_model(gdca_ctx *ctx, const void *W, const void *Z, int N, int M, int q)
{
    CHK(validate(ctx, N, M, q));
    if (!W || !Z) return fail(ctx, GDCA_EINVAL, "null pointer");
    return GDCA_OK;
}

static gdca_status check_plm_weights(gdca_ctx *ctx, const void *w, double Meff)
{
    if (!w) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (!(Meff > 0.0) || !std::isfinite(Meff)) return fail(ctx, GDCA_EINVAL, "invalid Meff");
    return GDCA_OK;
}

static gdca_status check_plm_tallies(gdca_ctx *ctx, const void *W, const void *Z, const void *w, double Meff, int N, int M, int q,
                                     const void *Pi_c, const void *Pij_c, const void *nll)
{
    CHK(check_plm_model(ctx, W, Z, N, M, q));
    CHK(check_plm_weights(ctx, w, Meff));
    if (!Pi_c || !Pij_c || !nll) return fail(ctx, GDCA_EINVAL, "null pointer");
    if (W == Pij_c || W == Pi_c || W == nll) return fail(ctx, GDCA_EINVAL, "W may not alias an output");
    return GDCA_OK;
}

static gdca_status check_plm_learn(gdca_ctx *ctx, const void *W, const void *Z, const void *w, double Meff, const void *Pi_d, const void *Pij_d,
                                   int N, int M, int q, int n_iter, double eta, double lambda, const void *trace)
{
    CHK(check_plm_model(ctx, W, Z, N, M, q));
    CHK(check_plm_weights(ctx, w, Meff));
    if (!Pi_d || !Pij_d || !trace) return fail(ctx, GDCA_EINVAL, "null pointer");
    CHK(check_bm_rates(ctx, eta, lambda));
    if (n_iter < 1) return fail(ctx, GDCA_EINVAL, "invalid n_iter");
    if (W == trace || W == Pij_d || W == Pi_d) return fail(ctx, GDCA_EINVAL, "W may not alias an output or the data's frequencies");
    return GDCA_OK;
}

// the weights' range, before anything is computed from them: one round trip
static gdca_status plm_weights_checked(gdca_ctx *ctx, const double *w_dev, int M)
{
    gdca_launch_plm_check_weights(ctx->stream, w_dev, M, (gdca_dev_scalars *)ctx->sc.p);
    CHK(check_launch(ctx, "weights check"));
    CHK(fetch_scalars(ctx));
    if (ctx->sc_host->bad_symbol & GDCA_BAD_WEIGHT) return fail(ctx, GDCA_EINVAL, "weights must lie in [0, 1]");
    return GDCA_OK;
}

// One pass over the M sequences Z (N x M) under (W, zero) in slabs: the potentials of a slab through the mutation stage -- into the
// caller's p where p_out is given, else into ctx->PLMv --, the softmax in place, l_ki into L, nll_k; and, where Q is given, the slab's
// tally into Q and S (+0.0 before the first slab: the caller's fill).
static gdca_status plm_pass(gdca_ctx *ctx, const double *W, const double *zero, const int8_t *Z, int N, int M, int q, const plm_geometry &g,
                            double *p_out, double *L, double *nll_k, const double *w, double *Q, double *S)
{
    const gdca_model model = operator_model(W, zero, N, q);
    const size_t seq = (size_t)N * q;
    if (!p_out) CHK(ensure(ctx, ctx->PLMv, (size_t)std::min(g.slab, M) * seq * sizeof(double)));
    for (int k0 = 0; k0 < M; k0 += g.slab) {
        const int cnt = std::min(g.slab, M - k0);
        double *D = p_out ? p_out + (size_t)k0 * seq : (double *)ctx->PLMv.p;
        CHK(mutation_stage(ctx, model, Z + (size_t)k0 * N, cnt, GDCA_MUT_POTENTIAL, D));
        gdca_launch_plm_softmax(ctx->stream, D, (const uint32_t *)ctx->Xg.p, N, cnt, q, L, nll_k + k0);
        if (Q) HIPCHK(gdca_launch_plm_tally(ctx->stream, D, (const uint32_t *)ctx->Xg.p, w + k0, N, q - 1, cnt, g.chunk, Q, S));
        CHK(check_launch(ctx, "pseudo-likelihood slab"));
    }
    return GDCA_OK;
}

// the conditional tallies and nll of (W, zero) into Pi_c, Pij_c, *nll: fill, the slabs, the finish, the weighted sum (ws: plm_plan's)
static gdca_status plm_tallies_stage(gdca_ctx *ctx, const double *W, const int8_t *Z, const double *w, double Meff, int N, int M, int q,
                                     const plm_geometry &g, const plm_plan &at, double *Pi_c, double *Pij_c, double *nll)
{
    hipStream_t s = ctx->stream;
    const int n = N * (q - 1);
    char *ws = (char *)ctx->PLMws.p;
    double *Q = (double *)(ws + at.q), *S = (double *)(ws + at.s), *zero = (double *)(ws + at.zero), *nllk = (double *)(ws + at.nllk),
           *L = (double *)(ws + at.l);
    gdca_launch_bm_fill(s, Q, (size_t)n * n, 0.0);
    gdca_launch_bm_fill(s, S, (size_t)n, 0.0);
    CHK(plm_pass(ctx, W, zero, Z, N, M, q, g, nullptr, L, nllk, w, Q, S));
    gdca_launch_plm_finish(s, Q, S, N, q - 1, Meff, Pi_c, Pij_c);
    gdca_launch_plm_nll(s, w, nllk, M, Meff, nll);
    return check_launch(ctx, "pseudo-likelihood tallies");
}

gdca_status gdca_plm_conditionals_dev(gdca_ctx *ctx, const double *W_dev, const int8_t *Z_dev, int32_t N, int32_t M, int32_t q, double *p_dev,
                                      double *nll_k_dev)
{
    CHK(check_plm_model(ctx, W_dev, Z_dev, N, M, q));
    if (!p_dev || !nll_k_dev) return fail(ctx, GDCA_EINVAL, "null pointer");
    if ((const void *)W_dev == p_dev || (const void *)W_dev == nll_k_dev) return fail(ctx, GDCA_EINVAL, "W may not alias an output");
    CHK(begin(ctx));
    const int n = N * (q - 1);
    const plm_geometry g(ctx, N, M, q);
    const plm_plan at(n, N, M, g.slab, false);
    CHK(ensure(ctx, ctx->PLMws, at.bytes));
    char *ws = (char *)ctx->PLMws.p;
    double *zero = (double *)(ws + at.zero);
    gdca_launch_bm_fill(ctx->stream, zero, (size_t)n, 0.0);
    CHK(plm_pass(ctx, W_dev, zero, Z_dev, N, M, q, g, p_dev, (double *)(ws + at.l), nll_k_dev, nullptr, nullptr, nullptr));
    return sequences_checked(ctx);
}

gdca_status gdca_plm_tally_dev(gdca_ctx *ctx, const double *p_dev, const int8_t *Z_dev, const double *w_dev, double Meff, int32_t N, int32_t M,
                               int32_t q, double *Pi_c_dev, double *Pij_c_dev)
{
    CHK(check_plm_model(ctx, p_dev, Z_dev, N, M, q));
    CHK(check_plm_weights(ctx, w_dev, Meff));
    if (!Pi_c_dev || !Pij_c_dev) return fail(ctx, GDCA_EINVAL, "null pointer");
    if ((const void *)p_dev == Pi_c_dev || (const void *)p_dev == Pij_c_dev) return fail(ctx, GDCA_EINVAL, "p may not alias an output");
    CHK(begin(ctx));
    CHK(plm_weights_checked(ctx, w_dev, M));
    hipStream_t s = ctx->stream;
    const int n = N * (q - 1);
    const plm_geometry g(ctx, N, M, q);
    const plm_plan at(n, N, M, g.slab, false);
    CHK(ensure(ctx, ctx->PLMws, at.bytes));
    CHK(ensure(ctx, ctx->Xg, (size_t)gdca_energy_blocks(N) * M * sizeof(uint32_t)));
    char *ws = (char *)ctx->PLMws.p;
    double *Q = (double *)(ws + at.q), *S = (double *)(ws + at.s);
    gdca_launch_energy_pack(s, Z_dev, (size_t)N, N, M, q, (uint32_t *)ctx->Xg.p, (gdca_dev_scalars *)ctx->sc.p);
    gdca_launch_bm_fill(s, Q, (size_t)n * n, 0.0);
    gdca_launch_bm_fill(s, S, (size_t)n, 0.0);
    HIPCHK(gdca_launch_plm_tally(s, p_dev, (const uint32_t *)ctx->Xg.p, w_dev, N, q - 1, M, g.chunk, Q, S));
    gdca_launch_plm_finish(s, Q, S, N, q - 1, Meff, Pi_c_dev, Pij_c_dev);
    CHK(check_launch(ctx, "pseudo-likelihood tally"));
    return sequences_checked(ctx);
}

gdca_status gdca_plm_tallies_dev(gdca_ctx *ctx, const double *W_dev, const int8_t *Z_dev, const double *w_dev, double Meff, int32_t N,
                                 int32_t M, int32_t q, double *Pi_c_dev, double *Pij_c_dev, double *nll_dev)
{
    CHK(check_plm_tallies(ctx, W_dev, Z_dev, w_dev, Meff, N, M, q, Pi_c_dev, Pij_c_dev, nll_dev));
    CHK(begin(ctx));
    CHK(plm_weights_checked(ctx, w_dev, M));
    const int n = N * (q - 1);
    const plm_geometry g(ctx, N, M, q);
    const plm_plan at(n, N, M, g.slab, false);
    CHK(ensure(ctx, ctx->PLMws, at.bytes));
    gdca_launch_bm_fill(ctx->stream, (double *)((char *)ctx->PLMws.p + at.zero), (size_t)n, 0.0);
    CHK(plm_tallies_stage(ctx, W_dev, Z_dev, w_dev, Meff, N, M, q, g, at, Pi_c_dev, Pij_c_dev, nll_dev));
    return sequences_checked(ctx);
}

gdca_status gdca_plm_learn_dev(gdca_ctx *ctx, double *W_dev, const int8_t *Z_dev, const double *w_dev, double Meff, const double *Pi_d_dev,
                               const double *Pij_d_dev, int32_t N, int32_t M, int32_t q, int32_t n_iter, double eta, double lambda,
                               double *trace_dev)
{
    CHK(check_plm_learn(ctx, W_dev, Z_dev, w_dev, Meff, Pi_d_dev, Pij_d_dev, N, M, q, n_iter, eta, lambda, trace_dev));
    CHK(begin(ctx));
    CHK(plm_weights_checked(ctx, w_dev, M));
    hipStream_t s = ctx->stream;
    const int n = N * (q - 1);
    const plm_geometry g(ctx, N, M, q);
    const plm_plan at(n, N, M, g.slab, true);
    CHK(ensure(ctx, ctx->PLMws, at.bytes));
    char *ws = (char *)ctx->PLMws.p;
    double *Pij_c = (double *)(ws + at.pij), *Pi_c = (double *)(ws + at.pi), *nll = (double *)(ws + at.nll);
    gdca_launch_bm_fill(s, (double *)(ws + at.zero), (size_t)n, 0.0);
    for (int it = 0; it < n_iter; ++it) {
        CHK(plm_tallies_stage(ctx, W_dev, Z_dev, w_dev, Meff, N, M, q, g, at, Pi_c, Pij_c, nll));
        double *out = trace_dev + 4 * (size_t)it;
        CHK(bm_readout_stage(ctx, Pi_d_dev, Pij_d_dev, Pi_c, Pij_c, N, q, out, false));
        HIPCHK(hipMemcpyAsync(out + 3, nll, sizeof(double), hipMemcpyDeviceToDevice, s));
        gdca_launch_bm_update(s, W_dev, Pij_d_dev, Pij_c, N, q - 1, eta, lambda);
        CHK(check_launch(ctx, "pseudo-likelihood iteration"));
    }
    return sequences_checked(ctx);  // (the sequences' flags, read once at the end)
}

gdca_status gdca_apc_dev(gdca_ctx *ctx, double *S_dev, int32_t N)
{
    if (!ctx || !S_dev || N < 1) return GDCA_EINVAL;
    CHK(not_pending(ctx));
    HIPCHK(hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->colsum, (size_t)N * sizeof(double)));
    gdca_launch_apc(ctx->stream, S_dev, N, (double *)ctx->colsum.p);
    return check_launch(ctx, "apc");
}

// ---- operator level, host pointers: copy in, run the `_dev` form, copy out --------------------------------------
// (what a statement-by-statement caller with ordinary Julia arrays binds; every n x n argument crosses PCIe, so a
// caller who chains several operators should keep the matrices in gdca_dbuf buffers and use the `_dev` forms)
// Each is: the checks of its `_dev` form (nothing is staged for a bad argument), a host_stage, one line per array, the `_dev` form, finish.

gdca_status gdca_pair_identity_sum(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, uint64_t *out)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z || !out) return GDCA_EINVAL;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    CHK(sg.status());
    return gdca_pair_identity_sum_dev(ctx, Z_dev, N, M, out);
}

gdca_status gdca_compute_theta(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, double *theta)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z || !theta) return GDCA_EINVAL;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    CHK(sg.status());
    return gdca_compute_theta_dev(ctx, Z_dev, N, M, theta);
}

gdca_status gdca_neighbour_counts(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, int32_t thresh,
                                  int32_t *n_out)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z || !n_out || thresh < 0) return GDCA_EINVAL;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    int32_t *n_dev = sg.out(n_out, (size_t)M * sizeof(int32_t));
    CHK(sg.status());
    return sg.finish(gdca_neighbour_counts_dev(ctx, Z_dev, N, M, thresh, n_dev));
}

gdca_status gdca_compute_weights(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, double theta, double *W,
                                 double *Meff, double *theta_used, int32_t *thresh)
{
    CHK(validate(ctx, N, M, 2));
    if (!Z || !W || !Meff || !(theta <= 1.0)) return GDCA_EINVAL;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    double *W_dev = sg.out(W, (size_t)M * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_compute_weights_dev(ctx, Z_dev, N, M, theta, W_dev, Meff, theta_used, thresh));
}

gdca_status gdca_frequencies(gdca_ctx *ctx, const int8_t *Z, int32_t N, int32_t M, int32_t q, const double *W,
                             double Meff, double *Pi, double *Pij)
{
    CHK(validate(ctx, N, M, q));
    if (!Z || !W || !Pi || !Pij || !(Meff > 0.0)) return GDCA_EINVAL;
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    const double *W_dev = sg.in(W, (size_t)M * sizeof(double));
    double *Pi_dev = sg.out(Pi, n * sizeof(double));
    double *Pij_dev = sg.out(Pij, n * n * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_frequencies_dev(ctx, Z_dev, N, M, q, W_dev, Meff, Pi_dev, Pij_dev));
}

gdca_status gdca_add_pseudocount(gdca_ctx *ctx, const double *Pi_true, const double *Pij_true, int32_t N, int32_t q,
                                 double pc, double *Pi, double *Pij)
{
    CHK(validate(ctx, N, 1, q));
    if (!Pi_true || !Pij_true || !Pi || !Pij || !(pc >= 0.0 && pc <= 1.0)) return GDCA_EINVAL;
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    // elementwise: in place on the device
    double *Pi_dev = sg.inout(Pi_true, Pi, n * sizeof(double));
    double *Pij_dev = sg.inout(Pij_true, Pij, n * n * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_add_pseudocount_dev(ctx, Pi_dev, Pij_dev, N, q, pc, Pi_dev, Pij_dev));
}

gdca_status gdca_covariance(gdca_ctx *ctx, const double *Pi, const double *Pij, int32_t n, double *C)
{
    if (!ctx || !Pi || !Pij || !C || n < 1 || n > GDCA_MAX_N) return GDCA_EINVAL;
    const size_t nn = (size_t)n;
    host_stage sg(ctx);
    const double *Pi_dev = sg.in(Pi, nn * sizeof(double));
    double *C_dev = sg.inout(Pij, C, nn * nn * sizeof(double));  // (C over Pij)
    CHK(sg.status());
    return sg.finish(gdca_covariance_dev(ctx, Pi_dev, C_dev, n, C_dev));
}

gdca_status gdca_spd_inverse(gdca_ctx *ctx, double *A, int32_t n, int32_t *info)
{
    if (!ctx || !A || n < 1 || n > GDCA_MAX_N) return GDCA_EINVAL;
    host_stage sg(ctx);
    double *A_dev = sg.inout(A, A, (size_t)n * n * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_spd_inverse_dev(ctx, A_dev, n, info));
}

gdca_status gdca_spd_inverse_logdet(gdca_ctx *ctx, double *A, int32_t n, int32_t *info, double *logdet)
{
    if (!ctx || !A || !logdet || n < 1 || n > GDCA_MAX_N) return GDCA_EINVAL;
    host_stage sg(ctx);
    double *A_dev = sg.inout(A, A, (size_t)n * n * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_spd_inverse_logdet_dev(ctx, A_dev, n, info, logdet));
}

gdca_status gdca_fn(gdca_ctx *ctx, const double *mJ, int32_t N, int32_t q, double *S)
{
    CHK(validate(ctx, N, 1, q));
    if (!mJ || !S) return GDCA_EINVAL;
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    double *S_dev = sg.out(S, (size_t)N * N * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_fn_dev(ctx, mJ_dev, N, q, S_dev));
}

gdca_status gdca_di(gdca_ctx *ctx, const double *mJ, const double *C, int32_t N, int32_t q, double *S)
{
    CHK(validate(ctx, N, 1, q));
    if (!mJ || !C || !S) return GDCA_EINVAL;
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *C_dev = sg.in(C, n * n * sizeof(double));
    double *S_dev = sg.out(S, (size_t)N * N * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_di_dev(ctx, mJ_dev, C_dev, N, q, S_dev));
}

gdca_status gdca_apc(gdca_ctx *ctx, double *S, int32_t N)
{
    if (!ctx || !S || N < 1) return GDCA_EINVAL;
    host_stage sg(ctx);
    double *S_dev = sg.inout(S, S, (size_t)N * N * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_apc_dev(ctx, S_dev, N));
}

gdca_status gdca_energies(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K, double *E)
{
    CHK(check_energies(ctx, mJ, Pi, N, q, X, K, E));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *X_dev = sg.in(X, (size_t)N * K);
    double *E_dev = sg.out(E, (size_t)K * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_energies_dev(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, E_dev));
}

gdca_status gdca_run_energies(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, const int8_t *X_host,
                              int32_t K, double *E_host, gdca_stats *st)
{
    CHK(check_run_energies(ctx, Z_host, N, M, q, p, X_host, K, E_host));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    double *E_dev = sg.out(E_host, (size_t)(X_host ? K : M) * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_energies_dev(ctx, Z_dev, N, M, q, p, X_dev, K, E_dev, st));
}

gdca_status gdca_run_loglik(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, const int8_t *X_host,
                            int32_t K, double *L_host, double *logdet, gdca_stats *st)
{
    CHK(check_run_energies(ctx, Z_host, N, M, q, p, X_host, K, L_host));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    double *L_dev = sg.out(L_host, (size_t)(X_host ? K : M) * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_loglik_dev(ctx, Z_dev, N, M, q, p, X_dev, K, L_dev, logdet, st));
}

gdca_status gdca_pair_energies(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, int32_t split, const int8_t *XA,
                               int32_t KA, const int8_t *XB, int32_t KB, int32_t what, double *E)
{
    CHK(check_pair_energies(ctx, mJ, Pi, N, q, split, XA, KA, XB, KB, what, E));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *XA_dev = sg.in(XA, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB, (size_t)(N - split) * KB);
    double *E_dev = sg.out(E, (size_t)KA * (size_t)KB * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_pair_energies_dev(ctx, mJ_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, what, E_dev));
}

gdca_status gdca_run_pair_energies(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                   const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, int32_t what, double *E_host,
                                   gdca_stats *st)
{
    CHK(check_run_pair(ctx, Z_host, N, M, q, p, split, XA_host, KA, XB_host, KB, what, E_host));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *XA_dev = sg.in(XA_host, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB_host, (size_t)(N - split) * KB);
    double *E_dev = sg.out(E_host, (size_t)(XA_host ? KA : M) * (size_t)(XB_host ? KB : M) * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_pair_energies_dev(ctx, Z_dev, N, M, q, p, split, XA_dev, KA, XB_dev, KB, what, E_dev, st));
}

gdca_status gdca_pair_energies_blocked(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, int32_t split, const int8_t *XA,
                                       int32_t KA, const int8_t *XB, int32_t KB, const void *offA, const void *offB, int32_t S, int32_t what,
                                       double *E)
{
    CHK(check_pair_energies(ctx, mJ, Pi, N, q, split, XA, KA, XB, KB, what, E));
    long long total = 0;
    CHK(check_blocks(ctx, offA, offB, S, KA, KB, &total));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *XA_dev = sg.in(XA, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB, (size_t)(N - split) * KB);
    double *E_dev = sg.out(E, (size_t)total * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_pair_energies_blocked_dev(ctx, mJ_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, offA, offB, S, what, E_dev));
}

gdca_status gdca_assign_blocks(gdca_ctx *ctx, const double *E, const void *offA, const void *offB, int32_t S, int32_t *match, double *gap)
{
    CHK(check_assign_blocks(ctx, E, offA, offB, S, match));
    const long long KA = ((const int32_t *)offA)[S], KB = ((const int32_t *)offB)[S];
    long long total = 0;
    CHK(check_blocks(ctx, offA, offB, S, KA, KB, &total));
    host_stage sg(ctx);
    const double *E_dev = sg.in(E, (size_t)total * sizeof(double));
    int32_t *match_dev = sg.out(match, (size_t)KA * sizeof(int32_t));
    double *gap_dev = sg.out(gap, (size_t)KA * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_assign_blocks_dev(ctx, E_dev, offA, offB, S, match_dev, gap_dev));
}

gdca_status gdca_run_partner_match(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                   const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, const void *offA, const void *offB,
                                   int32_t S, int32_t what, double *E_host, int32_t *match_host, double *gap_host, gdca_stats *st)
{
    const int ka = XA_host ? KA : M, kb = XB_host ? KB : M;
    CHK(check_run_partner(ctx, Z_host, N, M, q, p, split, ka, kb, offA, offB, what, match_host));
    long long total = 0;
    CHK(check_blocks(ctx, offA, offB, S, ka, kb, &total));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *XA_dev = sg.in(XA_host, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB_host, (size_t)(N - split) * KB);
    double *E_dev = sg.out(E_host, (size_t)total * sizeof(double));
    int32_t *match_dev = sg.out(match_host, (size_t)ka * sizeof(int32_t));
    double *gap_dev = sg.out(gap_host, (size_t)ka * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_partner_match_dev(ctx, Z_dev, N, M, q, p, split, XA_dev, KA, XB_dev, KB, offA, offB, S, what, E_dev, match_dev, gap_dev,
                                                st));
}

// pair log-odds with host pointers (three matrices cross PCIe in the operator forms)
static gdca_status logodds_operator_host(gdca_ctx *ctx, const double *mJ, const double *mJA, const double *mJB, const double *Pi, int32_t N, int32_t q,
                                         int32_t split, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, const void *offA,
                                         const void *offB, int32_t S, bool blocked, double I, double *L)
{
    CHK(check_pair_logodds(ctx, mJ, mJA, mJB, Pi, N, q, split, XA, KA, XB, KB, L));
    long long total = (long long)KA * KB;
    if (blocked) CHK(check_blocks(ctx, offA, offB, S, KA, KB, &total));
    const size_t s = (size_t)(q - 1), n = (size_t)N * s, nA = (size_t)split * s, nB = n - nA;
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *XA_dev = sg.in(XA, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB, (size_t)(N - split) * KB);
    const double *mJA_dev = sg.in(mJA, nA * nA * sizeof(double));
    const double *mJB_dev = sg.in(mJB, nB * nB * sizeof(double));
    double *L_dev = sg.out(L, (size_t)total * sizeof(double));
    CHK(sg.status());
    if (blocked)
        return sg.finish(
            gdca_pair_logodds_blocked_dev(ctx, mJ_dev, mJA_dev, mJB_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, offA, offB, S, I, L_dev));
    return sg.finish(gdca_pair_logodds_dev(ctx, mJ_dev, mJA_dev, mJB_dev, Pi_dev, N, q, split, XA_dev, KA, XB_dev, KB, I, L_dev));
}

gdca_status gdca_pair_logodds(gdca_ctx *ctx, const double *mJ, const double *mJA, const double *mJB, const double *Pi, int32_t N, int32_t q,
                              int32_t split, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, double I, double *L)
{
    return logodds_operator_host(ctx, mJ, mJA, mJB, Pi, N, q, split, XA, KA, XB, KB, nullptr, nullptr, 0, false, I, L);
}

gdca_status gdca_pair_logodds_blocked(gdca_ctx *ctx, const double *mJ, const double *mJA, const double *mJB, const double *Pi, int32_t N, int32_t q,
                                      int32_t split, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, const void *offA, const void *offB,
                                      int32_t S, double I, double *L)
{
    return logodds_operator_host(ctx, mJ, mJA, mJB, Pi, N, q, split, XA, KA, XB, KB, offA, offB, S, true, I, L);
}

gdca_status gdca_run_pair_logodds(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                  const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, double *L_host, double *EmA_host,
                                  double *EmB_host, double *info, gdca_stats *st)
{
    CHK(check_run_pair(ctx, Z_host, N, M, q, p, split, XA_host, KA, XB_host, KB, GDCA_PAIR_ENERGY, L_host));
    const size_t ka = (size_t)(XA_host ? KA : M), kb = (size_t)(XB_host ? KB : M);
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *XA_dev = sg.in(XA_host, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB_host, (size_t)(N - split) * KB);
    double *L_dev = sg.out(L_host, ka * kb * sizeof(double));
    double *EmA_dev = sg.out(EmA_host, ka * sizeof(double));
    double *EmB_dev = sg.out(EmB_host, kb * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_pair_logodds_dev(ctx, Z_dev, N, M, q, p, split, XA_dev, KA, XB_dev, KB, L_dev, EmA_dev, EmB_dev, info, st));
}

gdca_status gdca_run_partner_logodds(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p, int32_t split,
                                     const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, const void *offA, const void *offB,
                                     int32_t S, double *L_host, int32_t *match_host, double *gap_host, double *info, gdca_stats *st)
{
    const int ka = XA_host ? KA : M, kb = XB_host ? KB : M;
    CHK(check_run_partner(ctx, Z_host, N, M, q, p, split, ka, kb, offA, offB, GDCA_PAIR_ENERGY, match_host));
    long long total = 0;
    CHK(check_blocks(ctx, offA, offB, S, ka, kb, &total));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *XA_dev = sg.in(XA_host, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB_host, (size_t)(N - split) * KB);
    double *L_dev = sg.out(L_host, (size_t)total * sizeof(double));
    int32_t *match_dev = sg.out(match_host, (size_t)ka * sizeof(int32_t));
    double *gap_dev = sg.out(gap_host, (size_t)ka * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_partner_logodds_dev(ctx, Z_dev, N, M, q, p, split, XA_dev, KA, XB_dev, KB, offA, offB, S, L_dev, match_dev, gap_dev, info,
                                                  st));
}

gdca_status gdca_select_confident(gdca_ctx *ctx, const int32_t *match, const double *gap, int32_t KA, int32_t n_take, int32_t *sel, int32_t *n_sel)
{
    CHK(check_select_confident(ctx, match, gap, KA, sel));
    host_stage sg(ctx);
    const int32_t *match_dev = sg.in(match, (size_t)KA * sizeof(int32_t));
    const double *gap_dev = sg.in(gap, (size_t)KA * sizeof(double));
    int32_t *sel_dev = sg.out(sel, (size_t)KA * sizeof(int32_t));
    CHK(sg.status());
    return sg.finish(gdca_select_confident_dev(ctx, match_dev, gap_dev, KA, n_take, sel_dev, n_sel));
}

// (Z is the caller's whole alignment: only the requested columns are staged on the device and written back, and none where an index is bad)
gdca_status gdca_concat_pairs(gdca_ctx *ctx, const int8_t *XA, int32_t KA, const int8_t *XB, int32_t KB, int32_t N, int32_t split,
                              const int32_t *selA, const int32_t *selB, int32_t n_sel, int8_t *Z, int32_t col0)
{
    CHK(validate_concat(ctx, XA, KA, XB, KB, N, split, selA, selB, n_sel, Z, col0));
    if (n_sel == 0) return GDCA_OK;
    host_stage sg(ctx);
    const int8_t *XA_dev = sg.in(XA, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB, (size_t)(N - split) * KB);
    const int32_t *selA_dev = sg.in(selA, (size_t)n_sel * sizeof(int32_t));
    const int32_t *selB_dev = sg.in(selB, (size_t)n_sel * sizeof(int32_t));
    int8_t *Z_dev = sg.out(Z + (size_t)col0 * N, (size_t)N * n_sel);
    CHK(sg.status());
    return sg.finish(gdca_concat_pairs_dev(ctx, XA_dev, KA, XB_dev, KB, N, split, selA_dev, selB_dev, n_sel, Z_dev, 0));
}

gdca_status gdca_run_partner_ipa(gdca_ctx *ctx, const int8_t *XA_host, int32_t KA, const int8_t *XB_host, int32_t KB, const void *offA,
                                 const void *offB, int32_t S, int32_t N, int32_t q, int32_t split, int32_t what, const gdca_params *p,
                                 const int8_t *Zfix_host, int32_t Mfix, const int32_t *seedA, const int32_t *seedB, int32_t n_seed, int32_t n_inc,
                                 int32_t max_rounds, int32_t *match_host, double *gap_host, int32_t *match_trace_host, double *gap_trace_host,
                                 double *rounds_out, int32_t *rounds_run, gdca_stats *st)
{
    {
        ipa_plan plan;  // (the same checks before anything is staged: the sizes below are the caller's)
        CHK(ipa_check(ctx, KA, KB, offA, offB, S, N, q, split, what, p, Mfix, seedA, seedB, n_seed, n_inc, max_rounds, XA_host, XB_host, Zfix_host,
                      match_host, &plan));
    }
    const size_t nm = (size_t)KA * sizeof(int32_t), ng = (size_t)KA * sizeof(double);
    host_stage sg(ctx);
    const int8_t *Zfix_dev = Mfix > 0 ? sg.in(Zfix_host, (size_t)N * Mfix) : nullptr;
    const int8_t *XA_dev = sg.in(XA_host, (size_t)split * KA);
    const int8_t *XB_dev = sg.in(XB_host, (size_t)(N - split) * KB);
    // (device-only room: what comes back is the explicit fetches below)
    int32_t *match_dev = (int32_t *)sg.room(nm);
    double *gap_dev = (double *)sg.room(ng);
    int32_t *mt_dev = match_trace_host ? (int32_t *)sg.room(nm * max_rounds) : nullptr;
    double *gt_dev = gap_trace_host ? (double *)sg.room(ng * max_rounds) : nullptr;
    CHK(sg.status());
    int32_t done = 0;
    const gdca_status rs = gdca_run_partner_ipa_dev(ctx, XA_dev, KA, XB_dev, KB, offA, offB, S, N, q, split, what, p, Zfix_dev, Mfix, seedA, seedB,
                                                    n_seed, n_inc, max_rounds, match_dev, gap_dev, mt_dev, gt_dev, rounds_out, &done, st);
    if (rounds_run) *rounds_run = done;
    if (done > 0) {  // (the last completed round's, also where a later round's fit failed)
        sg.fetch(match_trace_host, mt_dev, nm * done);
        sg.fetch(gap_trace_host, gt_dev, ng * done);
        sg.fetch(gap_host, gap_dev, ng);
        sg.fetch(match_host, match_dev, nm);
        CHK(sg.finish(GDCA_OK));
    }
    return rs;
}

gdca_status gdca_mutation_scan(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                               int32_t what, double *D)
{
    CHK(check_mutation_scan(ctx, mJ, Pi, N, q, X, K, what, D));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *X_dev = sg.in(X, (size_t)N * K);
    double *D_dev = sg.out(D, (size_t)q * (size_t)N * (size_t)K * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_mutation_scan_dev(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, what, D_dev));
}

gdca_status gdca_run_mutation_scan(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                   const int8_t *X_host, int32_t K, int32_t what, double *D_host, gdca_stats *st)
{
    CHK(check_run_mutation_scan(ctx, Z_host, N, M, q, p, X_host, K, what, D_host));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    double *D_dev = sg.out(D_host, (size_t)q * (size_t)N * (size_t)(X_host ? K : M) * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_mutation_scan_dev(ctx, Z_dev, N, M, q, p, X_dev, K, what, D_dev, st));
}

gdca_status gdca_double_mutant_scan(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                                    double *Emin, int32_t *code, double *epi)
{
    CHK(check_double_scan(ctx, mJ, Pi, N, 1, q, X, K, Emin, code, epi));
    const size_t n = (size_t)N * (q - 1), maps = (size_t)N * (size_t)N * (size_t)K;
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *X_dev = sg.in(X, (size_t)N * K);
    double *Emin_dev = sg.out(Emin, maps * sizeof(double));
    int32_t *code_dev = sg.out(code, maps * sizeof(int32_t));
    double *epi_dev = sg.out(epi, maps * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_double_mutant_scan_dev(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, Emin_dev, code_dev, epi_dev));
}

gdca_status gdca_double_mutants(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                                const void *muts, int32_t L, double *out)
{
    CHK(check_double_list(ctx, mJ, Pi, N, 1, q, X, K, muts, L, out));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *X_dev = sg.in(X, (size_t)N * K);
    const void *muts_dev = sg.in(muts, (size_t)L * 5 * sizeof(int32_t));
    double *out_dev = sg.out(out, (size_t)L * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_double_mutants_dev(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, muts_dev, L, out_dev));
}

gdca_status gdca_run_double_mutant_scan(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                        const int8_t *X_host, int32_t K, double *Emin_host, int32_t *code_host, double *epi_host, gdca_stats *st)
{
    CHK(check_double_scan(ctx, Z_host, p, N, M, q, X_host, K, Emin_host, code_host, epi_host));
    const size_t maps = (size_t)N * (size_t)N * (size_t)K;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    double *Emin_dev = sg.out(Emin_host, maps * sizeof(double));
    int32_t *code_dev = sg.out(code_host, maps * sizeof(int32_t));
    double *epi_dev = sg.out(epi_host, maps * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_double_mutant_scan_dev(ctx, Z_dev, N, M, q, p, X_dev, K, Emin_dev, code_dev, epi_dev, st));
}

gdca_status gdca_run_double_mutants(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                    const int8_t *X_host, int32_t K, const void *muts_host, int32_t L, double *out_host, gdca_stats *st)
{
    CHK(check_double_list(ctx, Z_host, p, N, M, q, X_host, K, muts_host, L, out_host));
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    const void *muts_dev = sg.in(muts_host, (size_t)L * 5 * sizeof(int32_t));
    double *out_dev = sg.out(out_host, (size_t)L * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_double_mutants_dev(ctx, Z_dev, N, M, q, p, X_dev, K, muts_dev, L, out_dev, st));
}

gdca_status gdca_greedy_walk(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                             const int8_t *mask, int32_t flags, double min_gain, int32_t max_steps, int8_t *Xout, int32_t *steps,
                             double *dE_sum, int32_t *path, double *dE_path, double *V)
{
    CHK(check_greedy_walk(ctx, mJ, Pi, N, q, X, K, flags, min_gain, max_steps, Xout, steps));
    const size_t n = (size_t)N * (q - 1), k = (size_t)K, rows = (size_t)max_steps * k;
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *X_dev = sg.in(X, (size_t)N * k);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    int8_t *Xout_dev = sg.out(Xout, (size_t)N * k);
    int32_t *steps_dev = sg.out(steps, k * sizeof(int32_t));
    double *dE_sum_dev = sg.out(dE_sum, k * sizeof(double));
    int32_t *path_dev = sg.out(path, 2 * rows * sizeof(int32_t));
    double *dE_path_dev = sg.out(dE_path, rows * sizeof(double));
    double *V_dev = sg.out(V, (size_t)q * (size_t)N * k * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_greedy_walk_dev(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, mask_dev, flags, min_gain, max_steps, Xout_dev, steps_dev, dE_sum_dev,
                                          path_dev, dE_path_dev, V_dev));
}

gdca_status gdca_run_greedy_walk(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                 const int8_t *X_host, int32_t K, const int8_t *mask, int32_t flags, double min_gain, int32_t max_steps,
                                 int8_t *Xout, int32_t *steps, double *dE_sum, int32_t *path, double *dE_path, double *V, gdca_stats *st)
{
    CHK(check_run_greedy_walk(ctx, Z_host, N, M, q, p, X_host, K, flags, min_gain, max_steps, Xout, steps));
    const size_t k = (size_t)(X_host ? K : M), rows = (size_t)max_steps * k;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    int8_t *Xout_dev = sg.out(Xout, (size_t)N * k);
    int32_t *steps_dev = sg.out(steps, k * sizeof(int32_t));
    double *dE_sum_dev = sg.out(dE_sum, k * sizeof(double));
    int32_t *path_dev = sg.out(path, 2 * rows * sizeof(int32_t));
    double *dE_path_dev = sg.out(dE_path, rows * sizeof(double));
    double *V_dev = sg.out(V, (size_t)q * (size_t)N * k * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_greedy_walk_dev(ctx, Z_dev, N, M, q, p, X_dev, K, mask_dev, flags, min_gain, max_steps, Xout_dev, steps_dev,
                                              dE_sum_dev, path_dev, dE_path_dev, V_dev, st));
}

gdca_status gdca_sample(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *X, int32_t K,
                        const int8_t *mask, int32_t flags, double beta, uint64_t seed, uint64_t stream0, int32_t burn, int32_t stride,
                        int32_t n_samples, int8_t *Xs, double *dE_s, int32_t *accepted, double *thr, int32_t *moves, double *V)
{
    CHK(check_sample(ctx, mJ, Pi, N, q, X, K, flags, beta, burn, stride, n_samples, Xs, accepted));
    const size_t n = (size_t)N * (q - 1), k = (size_t)K, rows = ((size_t)burn + (size_t)n_samples * stride) * k;
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *X_dev = sg.in(X, (size_t)N * k);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    int8_t *Xs_dev = sg.out(Xs, (size_t)N * n_samples * k);
    double *dE_s_dev = sg.out(dE_s, (size_t)n_samples * k * sizeof(double));
    int32_t *accepted_dev = sg.out(accepted, k * sizeof(int32_t));
    double *thr_dev = sg.out(thr, rows * sizeof(double));
    int32_t *moves_dev = sg.out(moves, rows * sizeof(int32_t));
    double *V_dev = sg.out(V, (size_t)q * (size_t)N * k * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_sample_dev(ctx, mJ_dev, Pi_dev, N, q, X_dev, K, mask_dev, flags, beta, seed, stream0, burn, stride, n_samples, Xs_dev,
                                     dE_s_dev, accepted_dev, thr_dev, moves_dev, V_dev));
}

gdca_status gdca_run_sample(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                            const int8_t *X_host, int32_t K, const int8_t *mask, int32_t flags, double beta, uint64_t seed,
                            uint64_t stream0, int32_t burn, int32_t stride, int32_t n_samples, int8_t *Xs, double *dE_s, int32_t *accepted,
                            double *thr, int32_t *moves, double *V, gdca_stats *st)
{
    CHK(check_run_sample(ctx, Z_host, N, M, q, p, X_host, K, flags, beta, burn, stride, n_samples, Xs, accepted));
    const size_t k = (size_t)(X_host ? K : M), rows = ((size_t)burn + (size_t)n_samples * stride) * k;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    int8_t *Xs_dev = sg.out(Xs, (size_t)N * n_samples * k);
    double *dE_s_dev = sg.out(dE_s, (size_t)n_samples * k * sizeof(double));
    int32_t *accepted_dev = sg.out(accepted, k * sizeof(int32_t));
    double *thr_dev = sg.out(thr, rows * sizeof(double));
    int32_t *moves_dev = sg.out(moves, rows * sizeof(int32_t));
    double *V_dev = sg.out(V, (size_t)q * (size_t)N * k * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_run_sample_dev(ctx, Z_dev, N, M, q, p, X_dev, K, mask_dev, flags, beta, seed, stream0, burn, stride, n_samples,
                                         Xs_dev, dE_s_dev, accepted_dev, thr_dev, moves_dev, V_dev, st));
}

/* Log partition function with host pointers */
gdca_status gdca_log_partition(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *x, const int8_t *mask,
                               int32_t flags, const double *betas, int32_t L, int32_t sweep, int32_t K, uint64_t seed, uint64_t stream0,
                               double *out4, double *logw, double *E_end, int8_t *X0, int8_t *Xout, int32_t *accepted, double *thr,
                               int32_t *moves)
{
    CHK(check_log_partition(ctx, mJ, Pi, N, q, x, mask, flags, betas, L, sweep, K, out4, logw));
    const size_t n = (size_t)N * (q - 1), k = (size_t)K, rows = (size_t)L * (size_t)sweep * k;
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *x_dev = sg.in(x, (size_t)N);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    double *out4_dev = sg.out(out4, 4 * sizeof(double));
    double *logw_dev = sg.out(logw, k * sizeof(double));
    double *E_end_dev = sg.out(E_end, k * sizeof(double));
    int8_t *X0_dev = sg.out(X0, (size_t)N * k);
    int8_t *Xout_dev = sg.out(Xout, (size_t)N * k);
    int32_t *accepted_dev = sg.out(accepted, k * sizeof(int32_t));
    double *thr_dev = sg.out(thr, rows * sizeof(double));
    int32_t *moves_dev = sg.out(moves, rows * sizeof(int32_t));
    CHK(sg.status());
    return sg.finish(gdca_log_partition_dev(ctx, mJ_dev, Pi_dev, N, q, x_dev, mask_dev, flags, betas, L, sweep, K, seed, stream0, out4_dev, logw_dev,
                                            E_end_dev, X0_dev, Xout_dev, accepted_dev, thr_dev, moves_dev));
}

/* Replica-exchange chains with host pointers (fifteen arrays at the most: the pool has sixteen) */
gdca_status gdca_sample_tempered(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, const int8_t *Xr,
                                 const int32_t *slot0, int32_t K, int32_t R, const double *betas, const int8_t *mask, int32_t flags,
                                 uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride, int32_t n_samples,
                                 int8_t *Xs, double *E_s, int32_t *accepted, int32_t *swaps, int8_t *Xr_out, int32_t *slot_out, double *thr,
                                 int32_t *moves, double *swap_thr, int32_t *slot_path)
{
    CHK(check_sample_tempered(ctx, mJ, Pi, N, q, Xr, K, R, betas, flags, swap_every, burn, stride, n_samples, Xs, accepted, swaps, Xr_out,
                              slot_out));
    const size_t n = (size_t)N * (q - 1), k = (size_t)K, g = k * (size_t)R, n_steps = (size_t)burn + (size_t)n_samples * stride;
    const size_t pairs = k * (size_t)(R - 1), n_rounds = n_steps / (size_t)swap_every;
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    const int8_t *Xr_dev = sg.in(Xr, (size_t)N * g);
    const int32_t *slot0_dev = sg.in(slot0, g * sizeof(int32_t));
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    int8_t *Xs_dev = sg.out(Xs, (size_t)N * n_samples * k);
    double *E_s_dev = sg.out(E_s, (size_t)n_samples * k * sizeof(double));
    int32_t *accepted_dev = sg.out(accepted, g * sizeof(int32_t));
    int32_t *swaps_dev = pairs ? sg.out(swaps, pairs * sizeof(int32_t)) : (int32_t *)sg.room(sizeof(int32_t));  // (R == 1: nothing comes back)
    int8_t *Xr_out_dev = sg.out(Xr_out, (size_t)N * g);
    int32_t *slot_out_dev = sg.out(slot_out, g * sizeof(int32_t));
    double *thr_dev = sg.out(thr, n_steps * g * sizeof(double));
    int32_t *moves_dev = sg.out(moves, n_steps * g * sizeof(int32_t));
    double *swap_thr_dev = pairs && n_rounds ? sg.out(swap_thr, n_rounds * pairs * sizeof(double)) : nullptr;
    int32_t *slot_path_dev = n_rounds ? sg.out(slot_path, n_rounds * g * sizeof(int32_t)) : nullptr;
    CHK(sg.status());
    return sg.finish(gdca_sample_tempered_dev(ctx, mJ_dev, Pi_dev, N, q, Xr_dev, slot0_dev, K, R, betas, mask_dev, flags, seed, stream0, swap_every,
                                              burn, stride, n_samples, Xs_dev, E_s_dev, accepted_dev, swaps_dev, Xr_out_dev, slot_out_dev, thr_dev,
                                              moves_dev, swap_thr_dev, slot_path_dev));
}

gdca_status gdca_run_sample_tempered(gdca_ctx *ctx, const int8_t *Z_host, int32_t N, int32_t M, int32_t q, const gdca_params *p,
                                     const int8_t *X_host, int32_t K, int32_t R, const double *betas, const int8_t *mask, int32_t flags,
                                     uint64_t seed, uint64_t stream0, int32_t swap_every, int32_t burn, int32_t stride, int32_t n_samples,
                                     int8_t *Xs, double *E_s, int32_t *accepted, int32_t *swaps, int8_t *Xr_out, int32_t *slot_out,
                                     double *thr, int32_t *moves, double *swap_thr, int32_t *slot_path, gdca_stats *st)
{
    CHK(check_run_sample_tempered(ctx, Z_host, N, M, q, p, X_host, K, R, betas, flags, swap_every, burn, stride, n_samples, Xs, accepted, swaps,
                                  Xr_out, slot_out));
    const size_t k = (size_t)(X_host ? K : M), g = k * (size_t)R, n_steps = (size_t)burn + (size_t)n_samples * stride;
    const size_t pairs = k * (size_t)(R - 1), n_rounds = n_steps / (size_t)swap_every;
    host_stage sg(ctx);
    const int8_t *Z_dev = sg.in(Z_host, (size_t)N * M);
    const int8_t *X_dev = sg.in(X_host, (size_t)N * K);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    int8_t *Xs_dev = sg.out(Xs, (size_t)N * n_samples * k);
    double *E_s_dev = sg.out(E_s, (size_t)n_samples * k * sizeof(double));
    int32_t *accepted_dev = sg.out(accepted, g * sizeof(int32_t));
    int32_t *swaps_dev = pairs ? sg.out(swaps, pairs * sizeof(int32_t)) : (int32_t *)sg.room(sizeof(int32_t));
    int8_t *Xr_out_dev = sg.out(Xr_out, (size_t)N * g);
    int32_t *slot_out_dev = sg.out(slot_out, g * sizeof(int32_t));
    double *thr_dev = sg.out(thr, n_steps * g * sizeof(double));
    int32_t *moves_dev = sg.out(moves, n_steps * g * sizeof(int32_t));
    double *swap_thr_dev = pairs && n_rounds ? sg.out(swap_thr, n_rounds * pairs * sizeof(double)) : nullptr;
    int32_t *slot_path_dev = n_rounds ? sg.out(slot_path, n_rounds * g * sizeof(int32_t)) : nullptr;
    CHK(sg.status());
    return sg.finish(gdca_run_sample_tempered_dev(ctx, Z_dev, N, M, q, p, X_dev, K, R, betas, mask_dev, flags, seed, stream0, swap_every, burn,
                                                  stride, n_samples, Xs_dev, E_s_dev, accepted_dev, swaps_dev, Xr_out_dev, slot_out_dev, thr_dev,
                                                  moves_dev, swap_thr_dev, slot_path_dev, st));
}

/* Boltzmann-machine refinement with host pointers */
gdca_status gdca_potts_from_gaussian(gdca_ctx *ctx, const double *mJ, const double *Pi, int32_t N, int32_t q, double *W)
{
    CHK(check_potts(ctx, mJ, Pi, N, q, W));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *mJ_dev = sg.in(mJ, n * n * sizeof(double));
    const double *Pi_dev = sg.in(Pi, n * sizeof(double));
    double *W_dev = sg.out(W, n * n * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_potts_from_gaussian_dev(ctx, mJ_dev, Pi_dev, N, q, W_dev));
}

gdca_status gdca_bm_update(gdca_ctx *ctx, double *W, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int32_t N,
                           int32_t q, double eta, double lambda)
{
    (void)Pi_d, (void)Pi_m;
    CHK(check_bm_update(ctx, W, Pij_d, Pij_m, N, q, eta, lambda));
    const size_t nn = (size_t)N * (q - 1) * (size_t)N * (q - 1) * sizeof(double);
    host_stage sg(ctx);
    double *W_dev = sg.inout(W, W, nn);
    const double *Pij_d_dev = sg.in(Pij_d, nn);
    const double *Pij_m_dev = sg.in(Pij_m, nn);
    CHK(sg.status());
    return sg.finish(gdca_bm_update_dev(ctx, W_dev, nullptr, Pij_d_dev, nullptr, Pij_m_dev, N, q, eta, lambda));
}

gdca_status gdca_bm_readout(gdca_ctx *ctx, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int32_t N, int32_t q,
                            double *out4)
{
    CHK(check_bm_readout(ctx, Pi_d, Pij_d, Pi_m, Pij_m, N, q, out4));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *Pi_d_dev = sg.in(Pi_d, n * sizeof(double));
    const double *Pij_d_dev = sg.in(Pij_d, n * n * sizeof(double));
    const double *Pi_m_dev = sg.in(Pi_m, n * sizeof(double));
    const double *Pij_m_dev = sg.in(Pij_m, n * n * sizeof(double));
    double *out_dev = sg.out(out4, 4 * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_bm_readout_dev(ctx, Pi_d_dev, Pij_d_dev, Pi_m_dev, Pij_m_dev, N, q, out_dev));
}

gdca_status gdca_bm_learn(gdca_ctx *ctx, double *W, const double *Pi_d, const double *Pij_d, int32_t N, int32_t q, int8_t *X, int32_t K,
                          const int8_t *mask, int32_t flags, double beta, uint64_t seed, uint64_t iter0, int32_t n_iter, int32_t burn,
                          int32_t stride, int32_t n_samples, double eta, double lambda, double *trace, int8_t *Xs_last)
{
    CHK(check_bm_learn(ctx, W, Pi_d, Pij_d, N, q, X, K, flags, beta, iter0, n_iter, burn, stride, n_samples, eta, lambda, trace));
    const size_t n = (size_t)N * (q - 1), k = (size_t)K;
    host_stage sg(ctx);
    double *W_dev = sg.inout(W, W, n * n * sizeof(double));
    const double *Pi_d_dev = sg.in(Pi_d, n * sizeof(double));
    const double *Pij_d_dev = sg.in(Pij_d, n * n * sizeof(double));
    int8_t *X_dev = sg.inout(X, X, (size_t)N * k);
    const int8_t *mask_dev = sg.in(mask, (size_t)N);
    double *trace_dev = sg.out(trace, 4 * (size_t)n_iter * sizeof(double));
    int8_t *Xs_dev = sg.out(Xs_last, (size_t)N * n_samples * k);
    CHK(sg.status());
    return sg.finish(gdca_bm_learn_dev(ctx, W_dev, Pi_d_dev, Pij_d_dev, N, q, X_dev, K, mask_dev, flags, beta, seed, iter0, n_iter, burn, stride,
                                       n_samples, eta, lambda, trace_dev, Xs_dev));
}

/* pseudo-likelihood fit with host pointers */
gdca_status gdca_plm_conditionals(gdca_ctx *ctx, const double *W, const int8_t *Z, int32_t N, int32_t M, int32_t q, double *p, double *nll_k)
{
    CHK(check_plm_model(ctx, W, Z, N, M, q));
    if (!p || !nll_k) return fail(ctx, GDCA_EINVAL, "null pointer");
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *W_dev = sg.in(W, n * n * sizeof(double));
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    double *p_dev = sg.out(p, (size_t)M * N * q * sizeof(double));
    double *nll_k_dev = sg.out(nll_k, (size_t)M * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_plm_conditionals_dev(ctx, W_dev, Z_dev, N, M, q, p_dev, nll_k_dev));
}

gdca_status gdca_plm_tally(gdca_ctx *ctx, const double *p, const int8_t *Z, const double *w, double Meff, int32_t N, int32_t M, int32_t q,
                           double *Pi_c, double *Pij_c)
{
    CHK(check_plm_model(ctx, p, Z, N, M, q));
    CHK(check_plm_weights(ctx, w, Meff));
    if (!Pi_c || !Pij_c) return fail(ctx, GDCA_EINVAL, "null pointer");
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *p_dev = sg.in(p, (size_t)M * N * q * sizeof(double));
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    const double *w_dev = sg.in(w, (size_t)M * sizeof(double));
    double *Pi_dev = sg.out(Pi_c, n * sizeof(double));
    double *Pij_dev = sg.out(Pij_c, n * n * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_plm_tally_dev(ctx, p_dev, Z_dev, w_dev, Meff, N, M, q, Pi_dev, Pij_dev));
}

gdca_status gdca_plm_tallies(gdca_ctx *ctx, const double *W, const int8_t *Z, const double *w, double Meff, int32_t N, int32_t M, int32_t q,
                             double *Pi_c, double *Pij_c, double *nll)
{
    CHK(check_plm_tallies(ctx, W, Z, w, Meff, N, M, q, Pi_c, Pij_c, nll));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    const double *W_dev = sg.in(W, n * n * sizeof(double));
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    const double *w_dev = sg.in(w, (size_t)M * sizeof(double));
    double *Pi_dev = sg.out(Pi_c, n * sizeof(double));
    double *Pij_dev = sg.out(Pij_c, n * n * sizeof(double));
    double *nll_dev = sg.out(nll, sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_plm_tallies_dev(ctx, W_dev, Z_dev, w_dev, Meff, N, M, q, Pi_dev, Pij_dev, nll_dev));
}

gdca_status gdca_plm_learn(gdca_ctx *ctx, double *W, const int8_t *Z, const double *w, double Meff, const double *Pi_d, const double *Pij_d,
                           int32_t N, int32_t M, int32_t q, int32_t n_iter, double eta, double lambda, double *trace)
{
    CHK(check_plm_learn(ctx, W, Z, w, Meff, Pi_d, Pij_d, N, M, q, n_iter, eta, lambda, trace));
    const size_t n = (size_t)N * (q - 1);
    host_stage sg(ctx);
    double *W_dev = sg.inout(W, W, n * n * sizeof(double));
    const int8_t *Z_dev = sg.in(Z, (size_t)N * M);
    const double *w_dev = sg.in(w, (size_t)M * sizeof(double));
    const double *Pi_d_dev = sg.in(Pi_d, n * sizeof(double));
    const double *Pij_d_dev = sg.in(Pij_d, n * n * sizeof(double));
    double *trace_dev = sg.out(trace, 4 * (size_t)n_iter * sizeof(double));
    CHK(sg.status());
    return sg.finish(gdca_plm_learn_dev(ctx, W_dev, Z_dev, w_dev, Meff, Pi_d_dev, Pij_d_dev, N, M, q, n_iter, eta, lambda, trace_dev));
}

gdca_status gdca_probe_mfma_f64(gdca_ctx *ctx, int32_t iters, double *tflops)
{
    if (!ctx || !tflops || iters < 1) return GDCA_EINVAL;
    CHK(begin(ctx));
    hipStream_t s = ctx->stream;
    const int blocks = 256 * 2;  // 2 waves per SIMD, all resident at once
    host_stage sg(ctx);
    double *sink = (double *)sg.room((size_t)blocks * 256 * sizeof(double));
    CHK(sg.status());
    CHK(open_timeline(ctx, true, false));
    gdca_launch_probe_mfma_f64(s, sink, 16, blocks);  // warm-up
    CHK(mark(ctx, T_BEGIN));
    gdca_launch_probe_mfma_f64(s, sink, iters, blocks);
    CHK(mark(ctx, T_END));
    CHK(check_launch(ctx, "probe"));
    HIPCHK(hipStreamSynchronize(s));
    bool tfail = false;
    const double ms = elapsed(ctx, T_BEGIN, T_END, &tfail);
    if (tfail) return fail(ctx, GDCA_EHIP, "hipEventElapsedTime");
    const double flops = (double)blocks * 4.0 * (double)((iters + 1) / 2) * 16.0 * 2.0 * 16 * 16 * 4;  // 16 MFMAs per trip
    *tflops = flops / (ms * 1e-3) / 1e12;
    return GDCA_OK;
}

}  // extern "C"
