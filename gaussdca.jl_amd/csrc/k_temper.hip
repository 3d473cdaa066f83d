// Replica exchange (parallel tempering) over the Metropolis chains: every one of K chains runs R replicas, each a Metropolis chain of
// k_sample.hip's kind on a stream of its own, at the inverse temperature of the SLOT it holds (betas[slot]); after every swap_every
// proposals a swap round lets the holders of neighbouring slots exchange their slots by a Metropolis rule.  Only slot 0 is sampled.
// The rule in full is include/gdca.h's ("Replica-exchange chains").  States and tables never move: a swap exchanges two integers.
//
//   k_temper_init     one wave a chain: slot0 checked (a column that is no permutation of 0 .. R - 1 raises GDCA_BAD_SLOTS and the chain
//                     goes on with the identity, so nothing is ever indexed with a bad slot), the maps slot_of (replica -> slot) and
//                     holder (slot -> replica) written, the counts zeroed.
//   k_temper_chain    ONE workgroup a replica, k_sample's structure line for line: the proposal computed by every wave for itself on
//                     workgroup-uniform values, no barrier and no write on a rejected proposal, two barriers and the two-column update
//                     on an accepted one, the table in LDS (TL = true) or in place in HBM by the walk's placement rule.  What differs:
//                     beta is betas[slot_of[replica]] (fixed for the launch: slots change between launches only), the accepted
//                     proposals are added to the SLOT's count at the end of the launch (one replica holds a slot, so one thread
//                     writes a count), and no sample is written here.  A launch runs the proposals t0 .. t1 - 1, which never cross
//                     a round; between two launches the replica lives in HBM exactly as a plain chain does.
//   k_temper_round    one wave a chain, round e: thread p owns the pair (p, p + 1) where p % 2 == e % 2 -- the pairs of a round are
//                     disjoint, so each owner writes its two entries of either map and its own count --, then every thread r writes
//                     slot_path, and at a sample point the wave copies the symbols of slot 0's holder and its E0 + S out.  Integer
//                     and f64 scalar work, one log a pair.
//   k_temper_finish   the final symbols (1-based) and slots of every replica.
// COUPLING: replicas meet at launch boundaries only.  No persistent kernel, no flag between workgroups, nothing spins: a dependency
// that cannot hang is worth more than the microseconds a launch costs.
// ORDER-FIXED as k_sample: one thread an entry, one thread a sum, one thread a count, one thread a pair; the random numbers are
// functions of (seed, stream, counter).  No read-modify-write is shared between threads.
#include "gdca_internal.h"
#include "gdca_launch.h"

#include <climits>

struct k_temper_betas {
    double b[GDCA_TEMPER_MAX];
};

struct k_temper_args {
    const double *A;  // element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const uint32_t *Xg;      // [ceil(N / 4)][G]: the start symbols of the G = K R replicas (t0 == 0)
    double *V;               // [G][N][q]: the tables between two launches (the first: k_mut_rows', what = potential)
    const int8_t *mask;      // [N] or nullptr
    const int32_t *slot_of;  // [G]: the slot every replica holds during this launch
    int32_t *accepted;       // [K][R]: by slot
    double *thr;             // [G][n_steps] or nullptr
    int32_t *moves;          // [G][n_steps] or nullptr
    double *sum_state;       // [G]: the running sums between two launches
    unsigned char *x_state;  // [G][N]: the symbols between two launches
    unsigned long long seed, stream0;
    int N, sdim, G, R, gaps, n_steps, t0, t1;
    k_temper_betas betas;
};

#define TEMPER_G 0x9E3779B97F4A7C15ull

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <bool TL>
__global__ __launch_bounds__(256) void k_temper_chain(const k_temper_args p)
{
    extern __shared__ double lds_[];  // [TL ? N s : 0] the table's residue entries, then ints, shorts and bytes (k_sample's layout)
    const int N = p.N, sdim = p.sdim, q = sdim + 1, n = N * sdim;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t g = blockIdx.x;
    double *tabL = lds_;
    int *dec = reinterpret_cast<int *>(tabL + (TL ? n : 0));              // [4]: the length of the site list
    unsigned short *sites = reinterpret_cast<unsigned short *>(dec + 4);  // [N]: the sites that may change, ascending
    unsigned char *x = reinterpret_cast<unsigned char *>(sites + N);      // [N]
    double *Vg = p.V + g * (size_t)N * q;
    const bool first = p.t0 == 0;
    const int dj = 256 / sdim, dr = 256 - dj * sdim;  // row r + 256: site + dj, symbol + dr (mod s)
    const int slot = __builtin_amdgcn_readfirstlane(p.slot_of[g]);  // (k_temper_init: inside 0 .. R - 1)

    for (int i = t; i < N; i += 256)
        x[i] = first ? (unsigned char)((p.Xg[(size_t)(i >> 2) * p.G + g] >> (8 * (i & 3))) & 0xffu) : p.x_state[g * (size_t)N + i];
    if (TL) {
        int j = t / sdim, c = t - j * sdim;
        for (int r = t; r < n; r += 256) {
            tabL[r] = Vg[j * q + c];
            j += dj, c += dr;
            if (c >= sdim) c -= sdim, ++j;
        }
    }
    __syncthreads();
    // ---- the site list: wave 0, 64 sites at a time.  It is the START's list: without the flag a gap stays a gap and a residue a
    // residue, with it every site the mask lets change is listed, so the list of the current symbols is the list of the start
    if (wave == 0) {
        int cnt = 0;
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            const bool e = i < N && (!p.mask || p.mask[i] != 0) && (p.gaps || x[i] != sdim);
            const unsigned long long m = __ballot(e);
            if (e) sites[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)i;
            cnt += __popcll(m);
        }
        if (lane == 0) dec[0] = cnt;
    }
    __syncthreads();
    const int n_sites = __builtin_amdgcn_readfirstlane(dec[0]);
    auto ent = [&](int i, int c) -> double {
        if (!TL) return Vg[i * q + c];
        const double v = tabL[i * sdim + (c < sdim ? c : sdim - 1)];
        return c < sdim ? v : 0.0;
    };

    const unsigned long long T1 = (unsigned long long)(p.gaps ? q : sdim) - 1ull;  // T - 1 targets
    const unsigned long long key = mix64(mix64(p.seed + TEMPER_G) + (p.stream0 + g + 1ull) * TEMPER_G);  // the REPLICA's stream
    unsigned long long ctr = key + (2ull * (unsigned long long)p.t0 + 1ull) * TEMPER_G;                 // key + (c + 1) G of draw c = 2 t0
    const double *__restrict__ A = p.A;
    const size_t ld = p.ld;
    const double sign = p.sign, beta = p.betas.b[slot];
    const size_t row = g * (size_t)p.n_steps;
    int acc_n = 0;                               // this launch's accepted proposals (thread 0's is the one that is written)
    double sum = first ? 0.0 : p.sum_state[g];   // the accepted dE in step order

    for (int tt = p.t0; tt < p.t1; ++tt) {
        // ---- propose: every wave for itself, on uniform values
        const unsigned long long r0 = mix64(ctr), r1 = mix64(ctr + TEMPER_G);
        ctr += 2ull * TEMPER_G;
        const double u = (double)((r1 >> 11) + 1ull) * 0x1p-53;  // (0, 1], exact
        const double thr = -log(u);
        int code = INT_MIN, i = 0, a = 0, b = 0;
        double dE = 0.0;
        bool go = false;
        if (n_sites > 0) {
            i = sites[(int)(((r0 >> 32) * (unsigned long long)n_sites) >> 32)];
            const int v = (int)(((r0 & 0xffffffffull) * T1) >> 32);
            a = x[i];
            b = v + (v >= a);
            dE = ent(i, b) - ent(i, a);
            go = beta * dE <= thr;  // (false for a NaN on the left)
            code = i * q + b;
        }
        const int acc = __builtin_amdgcn_readfirstlane(go ? 1 : 0);
        if (t == 0) {
            if (p.thr) p.thr[row + tt] = thr;
            if (p.moves) p.moves[row + tt] = n_sites > 0 && !acc ? -1 - code : code;
        }
        // ---- accept: x_i, then the two columns r(i,b), r(i,a) into every other site's potentials
        if (acc) {
            i = __builtin_amdgcn_readfirstlane(i), a = __builtin_amdgcn_readfirstlane(a), b = __builtin_amdgcn_readfirstlane(b);
            sum = sum + dE;
            ++acc_n;
            __syncthreads();  // every wave has read the old state
            if (t == 0) x[i] = (unsigned char)b;
            const int rb = i * sdim + b, ra = i * sdim + a;  // (a gap has no column: not read)
            int j = t / sdim, c = t - j * sdim;
            for (int r = t; r < n; r += 256) {
                if (j != i) {
                    const double kb = b < sdim ? sign * A[r >= rb ? (size_t)rb * ld + r : (size_t)r * ld + rb] : 0.0;
                    const double ka = a < sdim ? sign * A[r >= ra ? (size_t)ra * ld + r : (size_t)r * ld + ra] : 0.0;
                    const double dk = kb - ka;
                    double &v = TL ? tabL[r] : Vg[j * q + c];
                    v = v + dk;
                }
                j += dj, c += dr;
                if (c >= sdim) c -= sdim, ++j;
            }
            __syncthreads();
        }
    }

    // ---- what the launch leaves for the next one and for the round: the symbols, the sum, the slot's count, the table
    for (int i = t; i < N; i += 256) p.x_state[g * (size_t)N + i] = x[i];
    if (t == 0) {
        p.sum_state[g] = sum;
        int32_t *cnt = p.accepted + (g / (size_t)p.R) * (size_t)p.R + slot;  // (this replica alone holds the slot)
        *cnt = *cnt + acc_n;
    }
    if (TL) {
        int j = t / sdim, c = t - j * sdim;
        for (int r = t; r < n; r += 256) {  // (the rows this thread updated)
            Vg[j * q + c] = tabL[r];
            j += dj, c += dr;
            if (c >= sdim) c -= sdim, ++j;
        }
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
            const unsigned long long key = mix64(mix64(p.seed + TEMPER_G) + (p.stream0 + base + 1ull) * TEMPER_G);
            const unsigned long long skey = mix64(~key);
            const unsigned long long c = (unsigned long long)e * (unsigned long long)R + (unsigned long long)t;
            const unsigned long long r1 = mix64(skey + (c + 1ull) * TEMPER_G);
            const double u = (double)((r1 >> 11) + 1ull) * 0x1p-53;
            th = -log(u);
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
    const size_t lds = gdca_sample_lds_bytes(N, sdim + 1, table_in_lds);
    // (gdca_api.hip checks before: walk_placement, validate_temper)
    if ((table_in_lds && !gdca_walk_table_fits(N, sdim + 1)) || lds > GDCA_WALK_LDS_LIMIT || N > 65535) return hipErrorInvalidValue;
    if (plan.R < 1 || plan.R > GDCA_TEMPER_MAX || plan.swap_every < 1) return hipErrorInvalidValue;
    const int n_steps = plan.burn + plan.n_samples * plan.stride;
    // a launch never crosses a round: the slots, and with them the temperatures, are fixed while it runs
    if (t0 < 0 || t1 <= t0 || t1 > n_steps || (t1 - 1) / plan.swap_every != t0 / plan.swap_every) return hipErrorInvalidValue;
    const int G = K * plan.R;
    const temper_state st(state, G);
    const k_temper_args a{A, ld, sign, Xg, V, plan.mask, st.slot_of, plan.accepted, plan.thr, plan.moves, st.sum, st.x, plan.seed, plan.stream0,
                          N, sdim, G, plan.R, (plan.flags & GDCA_SAMPLE_GAPS) != 0 ? 1 : 0, n_steps, t0, t1, betas_of(plan)};
    void (*kern)(k_temper_args) = table_in_lds ? k_temper_chain<true> : k_temper_chain<false>;
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)G), dim3(256), lds, s, a);
    return hipSuccess;
}

void gdca_launch_temper_round(hipStream_t s, int N, int K, const gdca_temper_plan &plan, int e, int js, void *state)
{
    const temper_state st(state, K * plan.R);
    const int n_rounds = (plan.burn + plan.n_samples * plan.stride) / plan.swap_every;
    const k_temper_round_args a{st.E0, st.sum, st.x, st.slot_of, st.holder, plan.swaps, plan.swap_thr, plan.slot_path, plan.Xs, plan.E_s,
                                plan.seed, plan.stream0, N, K, plan.R, e, n_rounds, js, plan.n_samples, betas_of(plan)};
    GDCA_LAUNCH_DIRECT(k_temper_round, dim3((unsigned)K), dim3(64), 0, s, a);
}

void gdca_launch_temper_finish(hipStream_t s, int N, int K, const gdca_temper_plan &plan, void *state)
{
    const temper_state st(state, K * plan.R);
    GDCA_LAUNCH_DIRECT(k_temper_finish, dim3((unsigned)K * (unsigned)plan.R), dim3(256), 0, s, st.x, st.slot_of, N, plan.Xr_out, plan.slot_out);
}
