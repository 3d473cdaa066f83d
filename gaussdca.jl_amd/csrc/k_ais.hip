// Log partition function by annealed importance sampling (Neal 2001): every one of K chains starts at a uniform draw from its state
// space, runs the Metropolis chain of k_sample.hip along a ladder of inverse temperatures betas[0] = 0 .. betas[L] and keeps the running
// log-weight of the path; |Omega| times the mean weight estimates Z(betas[L]).  The rule in full -- the starts, the stages, the weight
// step, the reduction -- is include/gdca.h's ("Log partition function"); the chain itself is csrc/gdca_chain.h's.
//
//   k_ais_start   one wave a chain: the site list of the template by ballot and popcount, 64 sites at a time (chain_run builds the
//                 same list from the start), the site at list position m takes the symbol of draw m of the chain's second stream,
//                 every other site keeps the template's.  A template byte outside 1..q is never free and is copied, so the pack of the
//                 energy stage reports it.
//   k_ais         ONE workgroup a chain: chain_run with the beta of the stage the proposal belongs to.  Its own:
//                   ladder   betas lives in HBM (a ladder is far longer than a kernel's arguments); the stage's beta is loaded once a
//                            stage, through a workgroup-uniform pointer that walks the ladder, and kept in a register between two
//                            stage ends (a stage counter beside the ladder's base and length cost three spilled SGPRs).
//                   weight   logw = logw + (betas[l-1] - betas[l]) * (E0 + S) ahead of stage l: once ahead of proposal 0, and in the
//                            hook behind the last proposal of stage l - 1.  Every thread carries logw (the same values in the same
//                            order), thread 0's is the one written.
//                   state    logw and the count lie beside the running sum between two launches, so a cut may fall anywhere.
//   k_ais_reduce  one workgroup: the maximum, the two sums of the shifted weights by 256 strided partials and a halving tree, out4.
// ORDER-FIXED as the chain body; the reduction's order is a function of K alone.
#include "gdca_chain.h"
#include "gdca_launch.h"

struct k_ais_start_args {
    const int8_t *x;     // [N] or nullptr: every site is free
    const int8_t *mask;  // [N] or nullptr
    int8_t *Xst;         // [K][N]: the starts, as the energy and the mutation stage take sequences
    int8_t *X0;          // [K][N] or nullptr
    int32_t *n_sites;    // the length of the site list (every chain's is the same: chain 0 writes it)
    unsigned long long seed, stream0;
    int N, q, gaps;
};

__global__ __launch_bounds__(64) void k_ais_start(const k_ais_start_args p)
{
    const int lane = threadIdx.x, N = p.N, q = p.q;
    const size_t k = blockIdx.x;
    const unsigned long long ikey = chain_swap_key(chain_key(p.seed, p.stream0 + k));
    const unsigned long long T = (unsigned long long)(p.gaps ? q : q - 1);
    int cnt = 0;  // (wave-uniform)
    for (int b0 = 0; b0 < N; b0 += 64) {
        const int i = b0 + lane;
        int sym = i < N && p.x ? p.x[i] : 1;
        const bool e = i < N && (!p.mask || p.mask[i] != 0) && (p.gaps || sym != q) && sym >= 1 && sym <= q;
        const unsigned long long m = __ballot(e);
        if (e) {
            const unsigned long long pos = (unsigned long long)(cnt + __popcll(m & ((1ull << lane) - 1ull)));
            const unsigned long long r = chain_mix64(chain_counter(ikey, pos));
            sym = 1 + (int)(((r >> 32) * T) >> 32);
        }
        if (i < N) {
            p.Xst[k * (size_t)N + i] = (int8_t)sym;
            if (p.X0) p.X0[k * (size_t)N + i] = (int8_t)sym;
        }
        cnt += __popcll(m);
    }
    if (lane == 0 && k == 0) *p.n_sites = cnt;
}

struct k_ais_args {
    chain_args c;
    const double *betas;  // [L + 1]
    const double *E0;     // [K]: the starts' energies
    double *logw_state;   // [K]: the log-weights between two launches
    int32_t *acc_state;   // [K]: the counts between two launches
    double *logw;         // [K]
    double *E_end;        // [K] or nullptr
    int8_t *Xout;         // [K][N] or nullptr
    int32_t *accepted;    // [K] or nullptr
    int sweep;
};

template <bool TL>
__global__ __launch_bounds__(256) void k_ais(const k_ais_args p)
{
    extern __shared__ double lds_[];  // chain_layout
    const int t = threadIdx.x, N = p.c.N, sweep = p.sweep, n_steps = p.c.n_steps;
    const size_t k = blockIdx.x;
    const double E0 = p.E0[k];
    const int l0 = p.c.t0 / sweep + 1;             // the stage of the launch's first proposal ...
    int next = l0 * sweep - 1;                     // ... that stage's last proposal (l0 sweep <= n_steps) ...
    const double *__restrict__ bp = p.betas + l0;  // ... and its beta
    double b_cur = *bp;
    double logw = 0.0, S = 0.0;
    if (p.c.t0 == 0) {
        const double E = E0 + S, d = p.betas[0] - b_cur;
        const double w = d * E;
        logw = logw + w;
    } else {
        logw = p.logw_state[k];
    }
    const int acc_n = chain_run<TL>(
        p.c, lds_, k, [&](int) { return b_cur; },
        [&](int tt, const unsigned char *, double sum) {
            S = sum;
            if (tt != next || tt + 1 == n_steps) return;
            // the weight step ahead of the next stage
            next += sweep;
            ++bp;
            const double bn = *bp, E = E0 + sum, d = b_cur - bn;
            const double w = d * E;
            logw = logw + w;
            b_cur = bn;
        });
    const bool last = p.c.t1 == n_steps;
    if (t == 0) {
        const int acc = (p.c.t0 == 0 ? 0 : p.acc_state[k]) + acc_n;
        p.acc_state[k] = acc;
        p.logw_state[k] = logw;
        if (last) {
            p.logw[k] = logw;
            if (p.E_end) p.E_end[k] = E0 + S;
            if (p.accepted) p.accepted[k] = acc;
        }
    }
    // (chain_run has just written x_state, every thread the entries it reads here)
    if (last && p.Xout)
        for (int i = t; i < N; i += 256) p.Xout[k * (size_t)N + i] = (int8_t)(p.c.x_state[k * (size_t)N + i] + 1);
}

// out[0] = log_omega + (m + log(S1 / K)), out[1] = S1 S1 / S2, out[2] = m, out[3] = log_omega; S1, S2 the sums of e_k = exp(logw[k] - m)
// and of e_k e_k: partial t the terms k = t, t + 256, .. ascending, the 256 partials folded by a halving tree (k_bm.hip's order)
__global__ __launch_bounds__(256) void k_ais_reduce(const double *__restrict__ logw, int K, const int32_t *__restrict__ n_sites, int T,
                                                    double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double r1[256], r2[256];
    __shared__ int bad_s[256];
    const int t = threadIdx.x;
    double mx = -INFINITY;
    int bad = 0;
    for (int k = t; k < K; k += 256) {
        const double v = logw[k];
        bad |= isfinite(v) ? 0 : 1;
        mx = fmax(mx, v);
    }
    r1[t] = mx;
    bad_s[t] = bad;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            r1[t] = fmax(r1[t], r1[t + w]);
            bad_s[t] = bad_s[t] | bad_s[t + w];
        }
        __syncthreads();
    }
    const double m = r1[0];
    bad = bad_s[0];
    __syncthreads();
    double s1 = 0.0, s2 = 0.0;
    for (int k = t; k < K; k += 256) {
        const double e = exp(logw[k] - m);
        const double ee = e * e;
        s1 = s1 + e;
        s2 = s2 + ee;
    }
    r1[t] = s1;
    r2[t] = s2;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            r1[t] = r1[t] + r1[t + w];
            r2[t] = r2[t] + r2[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double S1 = r1[0], S2 = r2[0];
        const double log_omega = (double)*n_sites * log((double)T);
        const double mean = S1 / (double)K;
        const double lz = m + log(mean);
        const double ss = S1 * S1;
        out[0] = bad ? NAN : log_omega + lz;
        out[1] = bad ? NAN : ss / S2;
        out[2] = m;
        out[3] = log_omega;
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
// the running sums, the log-weights and E0 (K doubles each), the counts (K int32), the length of the site list, then the symbols (K N bytes)
size_t gdca_ais_state_bytes(int N, int K)
{
    return (size_t)K * (3 * sizeof(double) + sizeof(int32_t)) + 2 * sizeof(int32_t) + (size_t)K * (size_t)N;
}

namespace {
struct ais_state {
    double *sum, *logw, *E0;
    int32_t *acc, *n_sites;
    unsigned char *x;
    ais_state(void *state, int K)
    {
        sum = reinterpret_cast<double *>(state);
        logw = sum + K;
        E0 = logw + K;
        acc = reinterpret_cast<int32_t *>(E0 + K);
        n_sites = acc + K;
        x = reinterpret_cast<unsigned char *>(n_sites + 2);
    }
};
}  // namespace

double *gdca_ais_E0(void *state, int K)
{
    return ais_state(state, K).E0;
}

void gdca_launch_ais_start(hipStream_t s, const int8_t *x, int N, int q, int K, const gdca_ais_plan &plan, int8_t *Xst, void *state)
{
    const k_ais_start_args a{x, plan.chain.mask, Xst, plan.X0, ais_state(state, K).n_sites, plan.chain.seed, plan.chain.stream0, N, q,
                             (plan.chain.flags & GDCA_SAMPLE_GAPS) != 0 ? 1 : 0};
    GDCA_LAUNCH_DIRECT(k_ais_start, dim3((unsigned)K), dim3(64), 0, s, a);
}

hipError_t gdca_launch_ais(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                           const gdca_ais_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state)
{
    size_t lds = 0;
    hipError_t e = gdca_chain_launch_check(N, sdim, table_in_lds, plan.chain, t0, t1, &lds);
    if (e != hipSuccess) return e;
    if (plan.L < 1 || plan.sweep < 1 || !plan.betas || !plan.logw) return hipErrorInvalidValue;
    const ais_state st(state, K);
    const k_ais_args a{chain_args_of(A, ld, sign, Xg, V, plan.chain, st.sum, st.x, N, sdim, K, t0, t1),
                       plan.betas, st.E0, st.logw, st.acc, plan.logw, plan.E_end, plan.Xout, plan.accepted, plan.sweep};
    void (*kern)(k_ais_args) = table_in_lds ? k_ais<true> : k_ais<false>;
    e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)K), dim3(256), lds, s, a);
    return hipSuccess;
}

void gdca_launch_ais_reduce(hipStream_t s, int K, int T, const gdca_ais_plan &plan, void *state)
{
    GDCA_LAUNCH_DIRECT(k_ais_reduce, dim3(1), dim3(256), 0, s, plan.logw, K, ais_state(state, K).n_sites, T, plan.out4);
}
