// Metropolis chains: every one of K chains proposes single substitutions of its sequence and accepts them at the inverse temperature
// beta, so that its states are drawn from exp(-beta E(x)) / Z over its state space.  The rule in full -- the state space, the
// counter-based SplitMix64, the proposal, `beta * dE <= -log(u)`, the sample points -- is include/gdca.h's ("Metropolis chains"); the
// chain itself -- its state, a step, what is ORDER-FIXED and why the bits do not depend on K, the placement or the cut into launches --
// is csrc/gdca_chain.h's.
//
//   k_sample  ONE workgroup a chain: chain_run at the launch's one beta (context option SAMPLE_CHUNK cuts the launches).  Its own:
//               sample   the hook behind every proposal: at a sample point all threads copy the symbols out, thread 0 the running sum.
//               count    `accepted` carries the chain's count from launch to launch: thread 0 adds this launch's.
#include "gdca_chain.h"
#include "gdca_launch.h"

struct k_sample_args {
    chain_args c;
    int8_t *Xs;         // [K][n_samples][N]
    double *dE_s;       // [K][n_samples] or nullptr
    int32_t *accepted;  // [K]
    double beta;
    int burn, stride, n_samples;
};

template <bool TL>
__global__ __launch_bounds__(256) void k_sample(const k_sample_args p)
{
    extern __shared__ double lds_[];  // chain_layout
    const int N = p.c.N, t = threadIdx.x;
    const size_t k = blockIdx.x;
    int js = p.c.t0 >= p.burn ? (p.c.t0 - p.burn) / p.stride : 0;             // the next sample ...
    long long next = (long long)p.burn + (long long)(js + 1) * p.stride - 1;  // ... is the state after this proposal
    const int acc_n = chain_run<TL>(p.c, lds_, k, p.beta, [&](int tt, const unsigned char *x, double sum) {
        if (tt != next) return;
        int8_t *out = p.Xs + (k * (size_t)p.n_samples + js) * (size_t)N;
        for (int s = t; s < N; s += 256) out[s] = (int8_t)(x[s] + 1);
        if (t == 0 && p.dE_s) p.dE_s[k * (size_t)p.n_samples + js] = sum;
        ++js;
        next += p.stride;
    });
    if (t == 0) p.accepted[k] = (p.c.t0 == 0 ? 0 : p.accepted[k]) + acc_n;
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------
size_t gdca_sample_state_bytes(int N, int K)
{
    return (size_t)K * sizeof(double) + (size_t)K * (size_t)N;
}

hipError_t gdca_chain_launch_check(int N, int sdim, bool table_in_lds, const gdca_chain_plan &c, int t0, int t1, size_t *lds)
{
    *lds = gdca_sample_lds_bytes(N, sdim + 1, table_in_lds);
    // (gdca_api.hip checks before: walk_placement, validate_sample)
    if ((table_in_lds && !gdca_walk_table_fits(N, sdim + 1)) || *lds > GDCA_WALK_LDS_LIMIT || N > 65535) return hipErrorInvalidValue;
    return t0 < 0 || t1 <= t0 || t1 > c.n_steps() ? hipErrorInvalidValue : hipSuccess;
}

hipError_t gdca_launch_sample(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                              const gdca_sample_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state)
{
    size_t lds = 0;
    hipError_t e = gdca_chain_launch_check(N, sdim, table_in_lds, plan.chain, t0, t1, &lds);
    if (e != hipSuccess) return e;
    double *sum_state = reinterpret_cast<double *>(state);
    const k_sample_args a{chain_args_of(A, ld, sign, Xg, V, plan.chain, sum_state, reinterpret_cast<unsigned char *>(sum_state + K), N, sdim, K, t0, t1),
                          plan.Xs, plan.dE_s, plan.accepted, plan.beta, plan.chain.burn, plan.chain.stride, plan.chain.n_samples};
    void (*kern)(k_sample_args) = table_in_lds ? k_sample<true> : k_sample<false>;
    e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)K), dim3(256), lds, s, a);
    return hipSuccess;
}
