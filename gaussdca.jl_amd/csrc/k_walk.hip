// Greedy walk: every one of K sequences descends the fitted Gaussian model's energy to a local minimum, one single substitution a step.
// With the site potentials V(x; i, c) of k_mutation.hip (V(x; i, gap) = +0.0) the energy change of setting site i to b is
//
//     dE(x; i, b) = V[i][b] - V[i][x_i]                                    (ONE f64 subtraction of two table entries)
//
// and once site i has gone from a to b every OTHER site's potentials change by two columns of mJ, its own not at all:
//
//     V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a)),  j != i, c in 1..s,     K(j,c; i,b) = mJ[r(j,c), r(i,b)], +0.0 where b is the gap
//
// (one subtraction, then one addition).  A step is O(N q) work a sequence where a fresh scan costs O(N n), and nothing leaves the
// device between two steps.  The rule in full -- admissible moves, the tie rule, the stop -- is include/gdca.h's ("greedy walk").
//
//   k_walk   ONE workgroup a sequence, persistent over its steps; no workgroup waits for another.  The state is the symbols x (bytes in
//            LDS, k_energy_pack's: 0 .. s, s = the gap) and the table V[i][c], q N doubles: in LDS (template TL = true; the table of
//            config C is 84 KB: one workgroup a compute unit) or left where the mutation stage wrote it in HBM (TL = false), updated in
//            place -- the same operations on the same values either way.  A step:
//              scan    thread t looks at the entries t, t + 256, .. of the table; entry idx = i q + (b - 1) IS the tie rule's code.  It
//                      keeps the smallest admissible (dE, code) of its share in the total order "dE, then code" (a NaN dE compares
//                      false and is never taken; +-0 compare equal and the code decides), the wave folds 64 of them with __shfl_xor,
//                      the four waves' go through LDS.  The order is total, so the tree does not matter.
//              decide  thread 0 folds the four, tests dE < -min_gain, records (i, b, dE), adds dE to its running sum, sets x_i and
//                      publishes (go, i, b, a) in LDS.  EVERY thread reads `go` there after the barrier (made a scalar: the loop's exit
//                      is workgroup-uniform, no lane leaves on a view of its own).
//              update  csrc/gdca_chain.h's chain_update: thread t takes the rows r = t, t + 256, .. of the two columns r(i,b), r(i,a)
//                      (the rows of site i left out).  The two columns of a step lie at most s doubles apart in the strided half, so
//                      they share most of their cache lines.  (No mirrored copy of the triangle is kept: 8 n^2 bytes of workspace for a
//                      read-side choice.)
//            Three barriers a step, none in a loop that lanes leave one by one.  A fused run's A holds -mJ (sign = -1): every load is
//            negated, which is exact, so both forms compute on the same values.
// ORDER-FIXED: every table entry is updated by one thread with the two operations above, the minimum is taken in a total order, the sum
// of the recorded dE is thread 0's in step order.  No floating-point atomics.  So a walk's outputs are the same bits from run to run,
// whatever K is, wherever x_k stands in the batch and wherever the table lives.
#include "gdca_chain.h"
#include "gdca_launch.h"

struct k_walk_args {
    const double *A;  // element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const uint32_t *Xg;  // [ceil(N / 4)][K]
    double *V;           // [K][N][q]: the initial table (k_mut_rows, what = potential); TL: written back if write_table, else updated in place
    const int8_t *mask;  // [N] or nullptr
    int8_t *Xout;        // [K][N]
    int32_t *steps;      // [K]
    double *dE_sum;      // [K] or nullptr
    int32_t *path;       // [K][max_steps][2] or nullptr
    double *dE_path;     // [K][max_steps] or nullptr
    double min_gain;
    int N, sdim, K, flags, max_steps, write_table;
};

// is (d2, c2) before (d, c) in the order "dE, then code"?  (false for a NaN d2; d is never NaN)
__device__ __forceinline__ bool walk_before(double d2, int c2, double d, int c)
{
    return d2 < d || (d2 == d && c2 < c);
}

template <bool TL>
__global__ __launch_bounds__(256) void k_walk(const k_walk_args p)
{
    extern __shared__ double lds_[];  // [4] the waves' minima, [TL ? N q : 0] the table, then ints and bytes
    const int N = p.N, sdim = p.sdim, q = sdim + 1, n = N * sdim, NQ = N * q;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t k = blockIdx.x;
    double *redD = lds_;
    double *tabL = lds_ + 4;
    int *redC = reinterpret_cast<int *>(tabL + (TL ? NQ : 0));  // [4]
    int *dec = redC + 4;                                         // go, i, b, a (symbols 0-based, sdim = the gap)
    unsigned char *x = reinterpret_cast<unsigned char *>(dec + 4);  // [N]
    unsigned char *ok = x + N;                                      // [N]: the mask lets site i change
    double *Vg = p.V + k * (size_t)NQ;

    for (int i = t; i < N; i += 256) {
        x[i] = (unsigned char)((p.Xg[(size_t)(i >> 2) * p.K + k] >> (8 * (i & 3))) & 0xffu);
        ok[i] = p.mask ? (p.mask[i] != 0) : 1;
    }
    if (TL)
        for (int idx = t; idx < NQ; idx += 256) tabL[idx] = Vg[idx];
    __syncthreads();
    // (one name for the table: an LDS pointer in one instance, a global one in the other)
    auto tab = [&](int idx) -> double & { return TL ? tabL[idx] : Vg[idx]; };

    const bool gap_target = (p.flags & GDCA_WALK_GAP_TARGET) != 0, fill_gaps = (p.flags & GDCA_WALK_FILL_GAPS) != 0;
    const double thresh = -p.min_gain;
    const int di = 256 / q, dc = 256 - di * q;  // entry idx + 256: site + di, symbol + dc (mod q)
    const double *__restrict__ A = p.A;
    const size_t ld = p.ld;
    const double sign = p.sign;
    const size_t prow = k * (size_t)p.max_steps;
    int nsteps = 0;      // (thread 0's count is the one that is written)
    double sum = 0.0;    // thread 0: the recorded dE in step order

    for (int step = 0; step < p.max_steps; ++step) {
        // ---- scan: the best admissible (dE, code) of this thread's entries
        double best = (double)INFINITY;
        int code = INT_MAX;
        {
            int i = t / q, c = t - i * q;
            for (int idx = t; idx < NQ; idx += 256) {
                const int a = x[i];
                const bool adm = ok[i] && c != a && (a != sdim || fill_gaps) && (c != sdim || gap_target);
                if (adm) {
                    const double d = tab(idx) - tab(i * q + a);
                    if (walk_before(d, idx, best, code)) best = d, code = idx;
                }
                i += di, c += dc;
                if (c >= q) c -= q, ++i;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double d2 = __shfl_xor(best, m);
            const int c2 = __shfl_xor(code, m);
            if (walk_before(d2, c2, best, code)) best = d2, code = c2;
        }
        if (lane == 0) redD[wave] = best, redC[wave] = code;
        __syncthreads();
        // ---- decide (one thread), publish
        if (t == 0) {
            for (int w = 1; w < 4; ++w)
                if (walk_before(redD[w], redC[w], best, code)) best = redD[w], code = redC[w];
            const int go = code != INT_MAX && best < thresh;
            dec[0] = go;
            if (go) {
                const int i = code / q, b = code - i * q;
                dec[1] = i, dec[2] = b, dec[3] = x[i];
                x[i] = (unsigned char)b;
                if (p.path) p.path[2 * (prow + step)] = i, p.path[2 * (prow + step) + 1] = b + 1;
                if (p.dE_path) p.dE_path[prow + step] = best;
                sum = sum + best;
                ++nsteps;
            }
        }
        __syncthreads();
        const int go = __builtin_amdgcn_readfirstlane(dec[0]);
        if (!go) break;
        // ---- update: the two columns r(i,b), r(i,a) into every other site's potentials
        {
            const int i = __builtin_amdgcn_readfirstlane(dec[1]), b = __builtin_amdgcn_readfirstlane(dec[2]),
                      a = __builtin_amdgcn_readfirstlane(dec[3]);
            chain_update(A, ld, sign, n, sdim, i, a, b, t, [&](int, int j, int c) -> double & { return tab(j * q + c); });
        }
        __syncthreads();
    }

    // ---- what the walk leaves: the final sequence, the counts, the unused rows of the path, the table
    if (t == 0) {
        dec[1] = nsteps;
        p.steps[k] = nsteps;
        if (p.dE_sum) p.dE_sum[k] = sum;
    }
    __syncthreads();
    const int first = dec[1];
    for (int i = t; i < N; i += 256) p.Xout[k * (size_t)N + i] = (int8_t)(x[i] + 1);
    for (int s = first + t; s < p.max_steps; s += 256) {
        if (p.path) p.path[2 * (prow + s)] = -1, p.path[2 * (prow + s) + 1] = -1;
        if (p.dE_path) p.dE_path[prow + s] = 0.0;
    }
    if (TL && p.write_table)
        for (int idx = t; idx < NQ; idx += 256) Vg[idx] = tabL[idx];
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------
// the dynamic LDS of the instance that keeps the table in LDS
size_t gdca_walk_lds_bytes(int N, int q, bool table_in_lds)
{
    const size_t b = (4 + (table_in_lds ? (size_t)N * q : 0)) * sizeof(double) + 8 * sizeof(int) + 2 * (size_t)N;
    return (b + 15) / 16 * 16;
}

bool gdca_walk_table_fits(int N, int q)
{
    return gdca_walk_lds_bytes(N, q, true) <= GDCA_WALK_LDS_LIMIT;
}

hipError_t gdca_launch_greedy_walk(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, int N, int sdim, int K,
                                   const int8_t *mask, int flags, double min_gain, int max_steps, double *V, bool table_in_lds, bool write_table,
                                   int8_t *Xout, int32_t *steps, double *dE_sum, int32_t *path, double *dE_path)
{
    if (table_in_lds && !gdca_walk_table_fits(N, sdim + 1)) return hipErrorInvalidValue;  // (gdca_api.hip checks before: walk_placement)
    const k_walk_args a{A, ld, sign, Xg, V, mask, Xout, steps, dE_sum, path, dE_path, min_gain, N, sdim, K, flags, max_steps, write_table ? 1 : 0};
    const size_t lds = gdca_walk_lds_bytes(N, sdim + 1, table_in_lds);
    void (*kern)(k_walk_args) = table_in_lds ? k_walk<true> : k_walk<false>;
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)K), dim3(256), lds, s, a);
    return hipSuccess;
}
