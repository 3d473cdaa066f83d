// Metropolis chains: every one of K chains proposes single substitutions of its sequence and accepts them at the inverse temperature
// beta, so that its states are drawn from exp(-beta E(x)) / Z over its state space.  The state is the walk's (k_walk.hip): the symbols
// x and the table of site potentials V[i][c], with
//
//     dE(x; i, b) = V[i][b] - V[i][x_i]                                    (ONE f64 subtraction of two table entries)
//     V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a)),  j != i, c in 1..s  (an accepted move from a to b at site i: the walk's two operations)
//
// and the rule in full -- the state space, the counter-based SplitMix64, the proposal, `beta * dE <= -log(u)`, the sample points -- is
// include/gdca.h's ("Metropolis chains").
//
//   k_sample  ONE workgroup a chain, as k_walk.  In LDS: the symbols (bytes, k_energy_pack's: 0 .. s, s = the gap), the ascending list
//             of the sites that may change (it cannot change along a chain), and -- template TL = true -- the table's N s residue
//             entries (the gap's entry is +0.0 and never written: it is in the code, so a table that fits the walk's LDS instance
//             fits this one: gdca_walk_table_fits); TL = false leaves the table where the mutation stage wrote it in HBM and updates
//             it in place -- the same operations on the same values either way.  What differs from the walk is the shape of a step:
//               propose  there is no scan.  Two mix64 of a counter, one list entry, one symbol, two table entries, one log, one
//                        compare -- all of them functions of workgroup-uniform values, so every wave computes the proposal for
//                        itself and all four reach the same verdict.  A REJECTED proposal takes no barrier and touches no memory
//                        beyond those reads; the waves may drift apart by any number of rejected proposals, which is harmless: nothing
//                        is written between two accepted moves.
//               accept   the verdict is made a scalar (readfirstlane: the branch is workgroup-uniform by construction), then one
//                        barrier (every wave has read the old state), thread 0 sets x_i, the walk's update pass over the two columns
//                        r(i,b), r(i,a) of the lower triangle (thread t: the rows t, t + 256, ..), one barrier.
//               record   thread 0 writes thr[t] and moves[t] where they are asked for; every thread carries the running sum and the
//                        count (the same values in the same order), thread 0's are the ones written.
//               sample   at a sample point all threads copy the symbols out: they are behind the second barrier of the last accepted
//                        move, and the next one's first barrier is ahead of every wave.
//             A launch runs the proposals t0 .. t1 - 1 (context option SAMPLE_CHUNK); between two launches the chain lives in HBM: the
//             symbols and the running sum in a workspace, the count in `accepted`, the table in V (written back bit for bit from LDS).
//             The generator is random-access, so the next launch resumes with the same numbers.
// ORDER-FIXED: every table entry is updated by one thread with the two operations above, the sum of the accepted dE is one thread's
// in step order, the random numbers are functions of (seed, stream, t).  No floating-point atomics.  So a chain's outputs are the same
// bits from run to run, whatever K is, wherever the chain stands in the batch, wherever the table lives and however the chain is cut
// into launches.
#include "gdca_internal.h"
#include "gdca_launch.h"

#include <climits>

struct k_sample_args {
    const double *A;  // element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const uint32_t *Xg;      // [ceil(N / 4)][K]: the start sequences (t0 == 0)
    double *V;               // [K][N][q]: the table between two launches (the first: k_mut_rows', what = potential)
    const int8_t *mask;      // [N] or nullptr
    int8_t *Xs;              // [K][n_samples][N]
    double *dE_s;            // [K][n_samples] or nullptr
    int32_t *accepted;       // [K]
    double *thr;             // [K][n_steps] or nullptr
    int32_t *moves;          // [K][n_steps] or nullptr
    double *sum_state;       // [K]: the running sum between two launches
    unsigned char *x_state;  // [K][N]: the symbols between two launches
    double beta;
    unsigned long long seed, stream0;
    int N, sdim, K, gaps, burn, stride, n_samples, n_steps, t0, t1;
};

#define SAMPLE_G 0x9E3779B97F4A7C15ull

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <bool TL>
__global__ __launch_bounds__(256) void k_sample(const k_sample_args p)
{
    extern __shared__ double lds_[];  // [TL ? N s : 0] the table's residue entries, then ints, shorts and bytes
    const int N = p.N, sdim = p.sdim, q = sdim + 1, n = N * sdim;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t k = blockIdx.x;
    double *tabL = lds_;
    int *dec = reinterpret_cast<int *>(tabL + (TL ? n : 0));                  // [4]: the length of the site list
    unsigned short *sites = reinterpret_cast<unsigned short *>(dec + 4);      // [N]: the sites that may change, ascending
    unsigned char *x = reinterpret_cast<unsigned char *>(sites + N);          // [N]
    double *Vg = p.V + k * (size_t)N * q;
    const bool first = p.t0 == 0;
    const int dj = 256 / sdim, dr = 256 - dj * sdim;  // row r + 256: site + dj, symbol + dr (mod s)

    for (int i = t; i < N; i += 256)
        x[i] = first ? (unsigned char)((p.Xg[(size_t)(i >> 2) * p.K + k] >> (8 * (i & 3))) & 0xffu) : p.x_state[k * (size_t)N + i];
    if (TL) {
        int j = t / sdim, c = t - j * sdim;
        for (int r = t; r < n; r += 256) {
            tabL[r] = Vg[j * q + c];
            j += dj, c += dr;
            if (c >= sdim) c -= sdim, ++j;
        }
    }
    __syncthreads();
    // ---- the site list: wave 0, 64 sites at a time (the count so far is wave-uniform)
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
    // (one name for an entry: the gap's is +0.0 in the LDS instance's code and in the HBM instance's memory)
    auto ent = [&](int i, int c) -> double {
        if (!TL) return Vg[i * q + c];
        const double v = tabL[i * sdim + (c < sdim ? c : sdim - 1)];
        return c < sdim ? v : 0.0;
    };

    const unsigned long long T1 = (unsigned long long)(p.gaps ? q : sdim) - 1ull;  // T - 1 targets
    const unsigned long long key = mix64(mix64(p.seed + SAMPLE_G) + (p.stream0 + k + 1ull) * SAMPLE_G);
    unsigned long long ctr = key + (2ull * (unsigned long long)p.t0 + 1ull) * SAMPLE_G;  // key + (c + 1) G of draw c = 2 t0
    const double *__restrict__ A = p.A;
    const size_t ld = p.ld;
    const double sign = p.sign, beta = p.beta;
    const size_t row = k * (size_t)p.n_steps;
    int acc_n = first ? 0 : p.accepted[k];       // (thread 0's are the ones that are written)
    double sum = first ? 0.0 : p.sum_state[k];   // the accepted dE in step order
    int js = p.t0 >= p.burn ? (p.t0 - p.burn) / p.stride : 0;                    // the next sample ...
    long long next = (long long)p.burn + (long long)(js + 1) * p.stride - 1;     // ... is the state after this proposal

    for (int tt = p.t0; tt < p.t1; ++tt) {
        // ---- propose: every wave for itself, on uniform values
        const unsigned long long r0 = mix64(ctr), r1 = mix64(ctr + SAMPLE_G);
        ctr += 2ull * SAMPLE_G;
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
                    // (r, col) of the symmetric matrix from its lower triangle: below the diagonal as it lies, above it mirrored
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
        // ---- sample: the state after proposal tt
        if (tt == next) {
            int8_t *out = p.Xs + (k * (size_t)p.n_samples + js) * (size_t)N;
            for (int s = t; s < N; s += 256) out[s] = (int8_t)(x[s] + 1);
            if (t == 0 && p.dE_s) p.dE_s[k * (size_t)p.n_samples + js] = sum;
            ++js;
            next += p.stride;
        }
    }

    // ---- what the launch leaves for the next one, and for the caller: the symbols, the sum, the count, the table
    for (int i = t; i < N; i += 256) p.x_state[k * (size_t)N + i] = x[i];
    if (t == 0) {
        p.sum_state[k] = sum;
        p.accepted[k] = acc_n;
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

// ---- launcher --------------------------------------------------------------------------------------------------------------------------
size_t gdca_sample_lds_bytes(int N, int q, bool table_in_lds)
{
    const size_t b = (table_in_lds ? (size_t)N * (q - 1) : 0) * sizeof(double) + 4 * sizeof(int) + 3 * (size_t)N;
    return (b + 15) / 16 * 16;
}

size_t gdca_sample_state_bytes(int N, int K)
{
    return (size_t)K * sizeof(double) + (size_t)K * (size_t)N;
}

hipError_t gdca_launch_sample(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                              const gdca_sample_plan &plan, int t0, int t1, double *V, bool table_in_lds, void *state)
{
    const size_t lds = gdca_sample_lds_bytes(N, sdim + 1, table_in_lds);
    // (gdca_api.hip checks before: walk_placement, validate_sample)
    if ((table_in_lds && !gdca_walk_table_fits(N, sdim + 1)) || lds > GDCA_WALK_LDS_LIMIT || N > 65535) return hipErrorInvalidValue;
    const int n_steps = plan.burn + plan.n_samples * plan.stride;
    if (t0 < 0 || t1 <= t0 || t1 > n_steps) return hipErrorInvalidValue;
    double *sum_state = reinterpret_cast<double *>(state);
    const k_sample_args a{A, ld, sign, Xg, V, plan.mask, plan.Xs, plan.dE_s, plan.accepted, plan.thr, plan.moves, sum_state,
                          reinterpret_cast<unsigned char *>(sum_state + K), plan.beta, plan.seed, plan.stream0, N, sdim, K,
                          (plan.flags & GDCA_SAMPLE_GAPS) != 0 ? 1 : 0, plan.burn, plan.stride, plan.n_samples, n_steps, t0, t1};
    void (*kern)(k_sample_args) = table_in_lds ? k_sample<true> : k_sample<false>;
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)K), dim3(256), lds, s, a);
    return hipSuccess;
}
