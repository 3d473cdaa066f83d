// Replica exchange (parallel tempering) over the Metropolis chains: every one of K chains runs R replicas, each a Metropolis chain of
// k_sample.hip's kind on a stream of its own, at the inverse temperature of the SLOT it holds (betas[slot]); after every swap_every
// proposals a swap round lets the holders of neighbouring slots exchange their slots by a Metropolis rule.  Only slot 0 is sampled.
// The rule in full is include/gdca.h's ("Replica-exchange chains").  States and tables never move: a swap exchanges two integers.
//
//   k_temper_init     one wave a chain: slot0 checked (a column that is no permutation of 0 .. R - 1 raises GDCA_BAD_SLOTS and the chain
//                     goes on with the identity, so nothing is ever indexed with a bad slot), the maps slot_of (replica -> slot) and
//                     holder (slot -> replica) written, the counts zeroed.
//   k_temper_chain    ONE workgroup a replica: csrc/gdca_chain.h's chain_run, the body k_sample runs -- no barrier and no write on a
//                     rejected proposal, two barriers and the two-column update on an accepted one, the table in LDS (TL = true) or in
//                     place in HBM by the walk's placement rule.  Its own: beta is betas[slot_of[replica]] (fixed for the launch: slots
//                     change between launches only), the accepted proposals are added to the SLOT's count at the end of the launch
//                     (one replica holds a slot, so one thread writes a count), and no sample is written here.  A launch runs the
//                     proposals t0 .. t1 - 1, which never cross a round; between two launches the replica lives in HBM exactly as a
//                     plain chain does.
//   k_temper_round    one wave a chain, round e: thread p owns the pair (p, p + 1) where p % 2 == e % 2 -- the pairs of a round are
//                     disjoint, so each owner writes its two entries of either map and its own count --, then every thread r writes
//                     slot_path, and at a sample point the wave copies the symbols of slot 0's holder and its E0 + S out.  Integer
//                     and f64 scalar work, one log a pair.
//   k_temper_finish   the final symbols (1-based) and slots of every replica.
// COUPLING: replicas meet at launch boundaries only.  No persistent kernel, no flag between workgroups, nothing spins: a dependency
// that cannot hang is worth more than the microseconds a launch costs.
// ORDER-FIXED as the chain body: one thread an entry, one thread a sum, one thread a count, one thread a pair; the random numbers are
// functions of (seed, stream, counter).  No read-modify-write is shared between threads.
#include "gdca_chain.h"
#include "gdca_launch.h"

struct k_temper_betas {
    double b[GDCA_TEMPER_MAX];
};

struct k_temper_args {
    chain_args c;            // G = K R replicas, the stream of replica g: stream0 + g
    const int32_t *slot_of;  // [G]: the slot every replica holds during this launch
    int32_t *accepted;       // [K][R]: by slot
    int R;
    k_temper_betas betas;
};

template <bool TL>
__global__ __launch_bounds__(256) void k_temper_chain(const k_temper_args p)
{
    extern __shared__ double lds_[];  // chain_layout
    const size_t g = blockIdx.x;
    const int slot = __builtin_amdgcn_readfirstlane(p.slot_of[g]);  // (k_temper_init: inside 0 .. R - 1)
    const int acc_n = chain_run<TL>(p.c, lds_, g, p.betas.b[slot], [](int, const unsigned char *, double) {});
    if (threadIdx.x == 0) {
        int32_t *cnt = p.accepted + (g / (size_t)p.R) * (size_t)p.R + slot;  // (this replica alone holds the slot)
        *cnt = *cnt + acc_n;
    }
}

// ---- the maps --------------------------------------------------------------------------------------------------------------------
struct k_temper_init_args {
    const int32_t *slot0;  // [K][R] or nullptr: the identity
    int32_t *slot_of, *holder, *accepted, *swaps;
    gdca_dev_scalars *sc;
    int K, R;
};

__global__ __launch_bounds__(64) void k_temper_init(const k_temper_init_args p)
{
    const int r = threadIdx.x, R = p.R;
    const size_t base = (size_t)blockIdx.x * R;
    int s = r;
    bool bad = false;
    if (r < R && p.slot0) {
        s = p.slot0[base + r];
        bad = s < 0 || s >= R;
        for (int o = 0; o < R && !bad; ++o) bad = o != r && p.slot0[base + o] == s;
    }
    if (__ballot(bad) != 0ull) {  // (one wave a chain: the verdict is the chain's)
        if (r == 0) p.sc->bad_symbol = p.sc->bad_symbol | GDCA_BAD_SLOTS;  // (no other kernel runs beside this one: every writer stores the same word)
        s = r;
    }
    if (r < R) {
        p.slot_of[base + r] = s;
        p.holder[base + s] = r;
        p.accepted[base + r] = 0;
        if (r < R - 1) p.swaps[(size_t)blockIdx.x * (R - 1) + r] = 0;
    }
}

struct k_temper_round_args {
    const double *E0, *sum_state;   // [G]
    const unsigned char *x_state;   // [G][N]
    int32_t *slot_of, *holder;      // [G]
    int32_t *swaps;                 // [K][R - 1]
    double *swap_thr;               // [K][R - 1][n_rounds] or nullptr
    int32_t *slot_path;             // [K][R][n_rounds] or nullptr
    int8_t *Xs;                     // [K][n_samples][N]
    double *E_s;                    // [K][n_samples] or nullptr
    unsigned long long seed, stream0;
    int N, K, R, e, n_rounds, js, n_samples;  // js: the sample this round is the point of, or -1
    k_temper_betas betas;
};

__global__ __launch_bounds__(64) void k_temper_round(const k_temper_round_args p)
{
    const int t = threadIdx.x, R = p.R, e = p.e;
    const size_t k = blockIdx.x, base = k * (size_t)R;
    if (t < R - 1) {
        double th = 0.0;  // (+0.0: the pair is not attempted in this round)
        if ((t & 1) == (e & 1)) {
            const int a = p.holder[base + t], b = p.holder[base + t + 1];
            const double Ea = p.E0[base + a] + p.sum_state[base + a];
            const double Eb = p.E0[base + b] + p.sum_state[base + b];
            const double db = p.betas.b[t] - p.betas.b[t + 1], dEab = Eb - Ea;
            const double d = db * dEab;
            const unsigned long long skey = chain_swap_key(chain_key(p.seed, p.stream0 + base));  // (the key of the chain's first replica)
            const unsigned long long c = (unsigned long long)e * (unsigned long long)R + (unsigned long long)t;
            th = chain_threshold(chain_uniform(chain_mix64(chain_counter(skey, c))));
            if (d <= th) {  // (false for a NaN; the pairs of a round are disjoint: these five words are this thread's)
                p.holder[base + t] = b;
                p.holder[base + t + 1] = a;
                p.slot_of[base + a] = t + 1;
                p.slot_of[base + b] = t;
                int32_t *cnt = p.swaps + k * (size_t)(R - 1) + t;
                *cnt = *cnt + 1;
            }
        }
        if (p.swap_thr) p.swap_thr[(k * (size_t)(R - 1) + t) * (size_t)p.n_rounds + e] = th;
    }
    __syncthreads();  // (the maps as the round leaves them)
    if (t < R && p.slot_path) p.slot_path[(base + t) * (size_t)p.n_rounds + e] = p.slot_of[base + t];
    if (p.js >= 0) {
        const size_t h = base + p.holder[base];
        int8_t *out = p.Xs + (k * (size_t)p.n_samples + p.js) * (size_t)p.N;
        for (int i = t; i < p.N; i += 64) out[i] = (int8_t)(p.x_state[h * (size_t)p.N + i] + 1);
        if (t == 0 && p.E_s) p.E_s[k * (size_t)p.n_samples + p.js] = p.E0[h] + p.sum_state[h];
    }
}

__global__ __launch_bounds__(256) void k_temper_finish(const unsigned char *x_state, const int32_t *slot_of, int N, int8_t *Xr_out,
                                                       int32_t *slot_out)
{
    const size_t g = blockIdx.x;
    for (int i = threadIdx.x; i < N; i += 256) Xr_out[g * (size_t)N + i] = (int8_t)(x_state[g * (size_t)N + i] + 1);
    if (threadIdx.x == 0) slot_out[g] = slot_of[g];
}

// Xr (N x R x K) <- every sequence of X (N x K), R times
__global__ __launch_bounds__(256) void k_temper_replicate(const int8_t *X, int N, int R, int8_t *Xr)
{
    const size_t g = blockIdx.x, k = g / (size_t)R;
    for (int i = threadIdx.x; i < N; i += 256) Xr[g * (size_t)N + i] = X[k * (size_t)N + i];
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
// the running sums and E0 (G doubles each), the two maps (G int32 each), then the symbols (G N bytes)
size_t gdca_temper_state_bytes(int N, int G)
{
    return (size_t)G * (2 * sizeof(double) + 2 * sizeof(int32_t)) + (size_t)G * (size_t)N;
}

namespace {
struct temper_state {
    double *sum, *E0;
    int32_t *slot_of, *holder;
    unsigned char *x;
    temper_state(void *state, int G)
    {
        sum = reinterpret_cast<double *>(state);
        E0 = sum + G;
        slot_of = reinterpret_cast<int32_t *>(E0 + G);
        holder = slot_of + G;
        x = reinterpret_cast<unsigned char *>(holder + G);
    }
};

k_temper_betas betas_of(const gdca_temper_plan &plan)
{
    k_temper_betas b{};
    for (int r = 0; r < plan.R; ++r) b.b[r] = plan.betas[r];
    return b;
}
}  // namespace

double *gdca_temper_E0(void *state, int G)
{
    return temper_state(state, G).E0;
}

void gdca_launch_temper_replicate(hipStream_t s, const int8_t *X, int N, int K, int R, int8_t *Xr)
{
    GDCA_LAUNCH_DIRECT(k_temper_replicate, dim3((unsigned)K * (unsigned)R), dim3(256), 0, s, X, N, R, Xr);
}

void gdca_launch_temper_init(hipStream_t s, const gdca_temper_plan &plan, int K, void *state, gdca_dev_scalars *sc)
{
    const temper_state st(state, K * plan.R);
    const k_temper_init_args a{plan.slot0, st.slot_of, st.holder, plan.accepted, plan.swaps, sc, K, plan.R};
    GDCA_LAUNCH_DIRECT(k_temper_init, dim3((unsigned)K), dim3(64), 0, s, a);
}

hipError_t gdca_launch_temper_chain(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                                    const gdca_temper_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state)
{
    size_t lds = 0;
    hipError_t e = gdca_chain_launch_check(N, sdim, table_in_lds, plan.chain, t0, t1, &lds);
    if (e != hipSuccess) return e;
    if (plan.R < 1 || plan.R > GDCA_TEMPER_MAX || plan.swap_every < 1) return hipErrorInvalidValue;
    // a launch never crosses a round: the slots, and with them the temperatures, are fixed while it runs
    if ((t1 - 1) / plan.swap_every != t0 / plan.swap_every) return hipErrorInvalidValue;
    const int G = K * plan.R;
    const temper_state st(state, G);
    const k_temper_args a{chain_args_of(A, ld, sign, Xg, V, plan.chain, st.sum, st.x, N, sdim, G, t0, t1), st.slot_of, plan.accepted, plan.R,
                          betas_of(plan)};
    void (*kern)(k_temper_args) = table_in_lds ? k_temper_chain<true> : k_temper_chain<false>;
    e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)G), dim3(256), lds, s, a);
    return hipSuccess;
}

void gdca_launch_temper_round(hipStream_t s, int N, int K, const gdca_temper_plan &plan, int e, int js, void *state)
{
    const temper_state st(state, K * plan.R);
    const k_temper_round_args a{st.E0, st.sum, st.x, st.slot_of, st.holder, plan.swaps, plan.swap_thr, plan.slot_path, plan.Xs, plan.E_s,
                                plan.chain.seed, plan.chain.stream0, N, K, plan.R, e, plan.chain.n_steps() / plan.swap_every, js,
                                plan.chain.n_samples, betas_of(plan)};
    GDCA_LAUNCH_DIRECT(k_temper_round, dim3((unsigned)K), dim3(64), 0, s, a);
}

void gdca_launch_temper_finish(hipStream_t s, int N, int K, const gdca_temper_plan &plan, void *state)
{
    const temper_state st(state, K * plan.R);
    GDCA_LAUNCH_DIRECT(k_temper_finish, dim3((unsigned)K * (unsigned)plan.R), dim3(256), 0, s, st.x, st.slot_of, N, plan.Xr_out, plan.slot_out);
}
