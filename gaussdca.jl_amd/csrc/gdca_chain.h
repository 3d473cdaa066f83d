// What the greedy walk (k_walk.hip), the Metropolis chains (k_sample.hip), the replica-exchange chains (k_temper.hip) and the annealed
// chains of the log partition function (k_ais.hip) share, each stated once: the counter-based generator, the two-column update of the
// table of site potentials, and -- the chain kernels' -- the LDS layout and the chain body (with, for their launchers, the fill of its
// arguments).  The rule in full is include/gdca.h's ("greedy walk", "Metropolis chains").
//
// The state is the symbols x (bytes, k_energy_pack's: 0 .. s, s = the gap) and the table V[i][c], with
//
//     dE(x; i, b) = V[i][b] - V[i][x_i]                                    (ONE f64 subtraction of two table entries)
//     V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a)),  j != i, c in 1..s  (an accepted move from a to b at site i: chain_update)
//
//   chain_run  ONE workgroup (256 threads) a chain.  In LDS (chain_layout): the symbols, the ascending list of the sites that may
//              change (it cannot change along a chain), and -- template TL = true -- the table's N s residue entries (the gap's entry is
//              +0.0 and never written: it is in the code, so a table that fits the walk's LDS instance fits this one:
//              gdca_walk_table_fits); TL = false leaves the table where the mutation stage wrote it in HBM and updates it in place -- the
//              same operations on the same values either way.  A step:
//                propose  there is no scan.  Two chain_mix64 of a counter, one list entry, one symbol, two table entries, one log, one
//                         compare -- all of them functions of workgroup-uniform values, so every wave computes the proposal for
//                         itself and all four reach the same verdict.  A REJECTED proposal takes no barrier and touches no memory
//                         beyond those reads; the waves may drift apart by any number of rejected proposals, which is harmless: nothing
//                         is written between two accepted moves.
//                accept   the verdict is made a scalar (readfirstlane: the branch is workgroup-uniform by construction), then one
//                         barrier (every wave has read the old state), thread 0 sets x_i, the update pass over the two columns
//                         r(i,b), r(i,a) of the lower triangle (thread t: the rows t, t + 256, ..), one barrier.
//                record   thread 0 writes thr[t] and moves[t] where they are asked for; every thread carries the running sum and the
//                         count (the same values in the same order), thread 0's are the ones written.
//                after    the caller's hook behind every proposal, on all threads: they are behind the second barrier of the last
//                         accepted move, and the next one's first barrier is ahead of every wave, so it may read the symbols.
//              A launch runs the proposals t0 .. t1 - 1; between two launches the chain lives in HBM: the symbols and the running sum in
//              a workspace, the table in V (written back bit for bit from LDS).  The generator is random-access, so the next launch
//              resumes with the same numbers.
// ORDER-FIXED: every table entry is updated by one thread with the two operations above, the sum of the accepted dE is one thread's
// in step order, the count is one thread's, the random numbers are functions of (seed, stream, counter).  No floating-point atomics,
// no read-modify-write shared between threads.  So a chain's outputs are the same bits from run to run, wherever the chain stands in
// the batch, wherever the table lives and however the chain is cut into launches.
#pragma once
#include "gdca_internal.h"

#include <climits>

// ---- the generator: SplitMix64 by counter -- draw c of a stream is chain_mix64(key + (c + 1) G) ---------------------------------------------------
constexpr unsigned long long CHAIN_G = 0x9E3779B97F4A7C15ull;  // 2^64 / the golden ratio

__device__ __forceinline__ unsigned long long chain_mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long chain_key(unsigned long long seed, unsigned long long stream)
{
    return chain_mix64(chain_mix64(seed + CHAIN_G) + (stream + 1ull) * CHAIN_G);
}

// the key of a stream of its own beside a chain's proposals (k_temper_round's swaps)
__device__ __forceinline__ unsigned long long chain_swap_key(unsigned long long key)
{
    return chain_mix64(~key);
}

// what chain_mix64 takes for draw c (the draw behind it: + CHAIN_G)
__device__ __forceinline__ unsigned long long chain_counter(unsigned long long key, unsigned long long c)
{
    return key + (c + 1ull) * CHAIN_G;
}

// a draw's uniform in (0, 1], exact, and the threshold an energy difference is held against
__device__ __forceinline__ double chain_uniform(unsigned long long r)
{
    return (double)((r >> 11) + 1ull) * 0x1p-53;
}

__device__ __forceinline__ double chain_threshold(double u)
{
    return -log(u);
}

// ---- the two-column update ------------------------------------------------------------------------------------------------------------------
// f(r, j, c) for the rows r = t, t + 256, .. < n of one thread: r = j sdim + c
template <class F>
__device__ __forceinline__ void chain_rows(int n, int sdim, int t, F f)
{
    const int dj = 256 / sdim, dr = 256 - dj * sdim;  // row r + 256: site + dj, symbol + dr (mod s)
    int j = t / sdim, c = t - j * sdim;
    for (int r = t; r < n; r += 256) {
        f(r, j, c);
        j += dj, c += dr;
        if (c >= sdim) c -= sdim, ++j;
    }
}

// Site i has gone from a to b: the two columns r(i,b), r(i,a) into every OTHER site's potentials, one subtraction, then one addition.
// at(r, j, c): the table's entry of row r = (j, c), wherever and however it is kept.  sign = -1: A holds -mJ and every load is negated,
// which is exact.  mJ is symmetric and only its lower triangle is read: the rows below the column's diagonal element are contiguous,
// the rows above it are a walk with stride ld along ROW r(i, .) (DESIGN 3.8b has the measured cost of the strided half).
template <class At>
__device__ __forceinline__ void chain_update(const double *__restrict__ A, size_t ld, double sign, int n, int sdim, int i, int a, int b, int t,
                                             At at)
{
    const int rb = i * sdim + b, ra = i * sdim + a;  // (a gap has no column: not read)
    chain_rows(n, sdim, t, [&](int r, int j, int c) {
        if (j == i) return;
        // (r, col) of the symmetric matrix from its lower triangle: below the diagonal as it lies, above it mirrored
        const double kb = b < sdim ? sign * A[r >= rb ? (size_t)rb * ld + r : (size_t)r * ld + rb] : 0.0;
        const double ka = a < sdim ? sign * A[r >= ra ? (size_t)ra * ld + r : (size_t)r * ld + ra] : 0.0;
        const double dk = kb - ka;
        double &v = at(r, j, c);
        v = v + dk;
    });
}

// ---- the chains' LDS layout: byte offsets into the launch's dynamic LDS ----------------------------------------------------------------------
struct chain_layout {
    size_t dec;    // int [4]: the length of the site list (the table's [TL ? N s : 0] doubles lie ahead of it, at 0)
    size_t sites;  // unsigned short [N]: the sites that may change, ascending
    size_t x;      // unsigned char [N]: the symbols
    size_t end;
};

__host__ __device__ inline chain_layout chain_layout_of(int N, int sdim, bool table_in_lds)
{
    chain_layout l;
    l.dec = (table_in_lds ? (size_t)N * sdim : 0) * sizeof(double);
    l.sites = l.dec + 4 * sizeof(int);
    l.x = l.sites + (size_t)N * sizeof(unsigned short);
    l.end = l.x + (size_t)N;
    return l;
}

__host__ __device__ inline size_t gdca_sample_lds_bytes(int N, int q, bool table_in_lds)
{
    return (chain_layout_of(N, q - 1, table_in_lds).end + 15) / 16 * 16;
}

// ---- the chain body -------------------------------------------------------------------------------------------------------------------------
struct chain_args {
    const double *A;  // element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const uint32_t *Xg;      // [ceil(N / 4)][G]: the start sequences (t0 == 0)
    double *V;               // [G][N][q]: the tables between two launches (the first: k_mut_rows', what = potential)
    const int8_t *mask;      // [N] or nullptr
    double *thr;             // [G][n_steps] or nullptr
    int32_t *moves;          // [G][n_steps] or nullptr
    double *sum_state;       // [G]: the running sums between two launches
    unsigned char *x_state;  // [G][N]: the symbols between two launches
    unsigned long long seed, stream0;
    int N, sdim, G, gaps, n_steps, t0, t1;  // G: the chains of the launch, one workgroup each
};

// the inverse temperature of proposal tt: a chain's one beta, or a workgroup-uniform function of tt (k_ais.hip: a ladder's stage)
__device__ __forceinline__ double beta_at(double beta, int)
{
    return beta;
}

template <class F>
__device__ __forceinline__ double beta_at(const F &beta, int tt)
{
    return beta(tt);
}

// The proposals t0 .. t1 - 1 of chain g at the inverse temperature beta_at(beta, tt); after(tt, x, sum) behind proposal tt.  -> the
// proposals this launch accepted (every thread's count is the same)
template <bool TL, class Beta, class After>
__device__ __forceinline__ int chain_run(const chain_args &p, double *lds, size_t g, Beta beta, After after)
{
    const int N = p.N, sdim = p.sdim, q = sdim + 1, n = N * sdim;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const chain_layout lay = chain_layout_of(N, sdim, TL);
    unsigned char *base = reinterpret_cast<unsigned char *>(lds);
    double *tabL = lds;
    int *dec = reinterpret_cast<int *>(base + lay.dec);
    unsigned short *sites = reinterpret_cast<unsigned short *>(base + lay.sites);
    unsigned char *x = base + lay.x;
    double *Vg = p.V + g * (size_t)N * q;
    const bool first = p.t0 == 0;

    for (int i = t; i < N; i += 256)
        x[i] = first ? (unsigned char)((p.Xg[(size_t)(i >> 2) * p.G + g] >> (8 * (i & 3))) & 0xffu) : p.x_state[g * (size_t)N + i];
    if (TL) chain_rows(n, sdim, t, [&](int r, int j, int c) { tabL[r] = Vg[j * q + c]; });
    __syncthreads();
    // ---- the site list: wave 0, 64 sites at a time (the count so far is wave-uniform).  It is the START's list: without the flag a gap
    // stays a gap and a residue a residue, with it every site the mask lets change is listed, so the list of the current symbols is
    // the list of the start
    if (wave == 0) {
        int cnt = 0;
        for (int b0 = 0; b0 < N; b0 += 64) {
            const int i = b0 + lane;
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
    unsigned long long ctr = chain_counter(chain_key(p.seed, p.stream0 + g), 2ull * (unsigned long long)p.t0);  // draw c = 2 t0
    const double *__restrict__ A = p.A;
    const size_t ld = p.ld;
    const double sign = p.sign;
    const size_t row = g * (size_t)p.n_steps;
    int acc_n = 0;                              // (thread 0's is the one that is written)
    double sum = first ? 0.0 : p.sum_state[g];  // the accepted dE in step order

    for (int tt = p.t0; tt < p.t1; ++tt) {
        // ---- propose: every wave for itself, on uniform values
        const unsigned long long r0 = chain_mix64(ctr), r1 = chain_mix64(ctr + CHAIN_G);
        ctr += 2ull * CHAIN_G;
        const double thr = chain_threshold(chain_uniform(r1));
        int code = INT_MIN, i = 0, a = 0, b = 0;
        double dE = 0.0;
        bool go = false;
        if (n_sites > 0) {
            i = sites[(int)(((r0 >> 32) * (unsigned long long)n_sites) >> 32)];
            const int v = (int)(((r0 & 0xffffffffull) * T1) >> 32);
            a = x[i];
            b = v + (v >= a);
            dE = ent(i, b) - ent(i, a);
            go = beta_at(beta, tt) * dE <= thr;  // (false for a NaN on the left)
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
            chain_update(A, ld, sign, n, sdim, i, a, b, t, [&](int r, int j, int c) -> double & { return TL ? tabL[r] : Vg[j * q + c]; });
            __syncthreads();
        }
        after(tt, x, sum);
    }

    // ---- what the launch leaves for the next one, and for the caller: the symbols, the sum, the table
    for (int i = t; i < N; i += 256) p.x_state[g * (size_t)N + i] = x[i];
    if (t == 0) p.sum_state[g] = sum;
    if (TL) chain_rows(n, sdim, t, [&](int r, int j, int c) { Vg[j * q + c] = tabL[r]; });  // (the rows this thread updated)
    return acc_n;
}

// ---- host: the kernel's arguments from a plan (the launchers' shared checks: gdca_chain_launch_check, gdca_internal.h) ---------------------------
inline chain_args chain_args_of(const double *A, size_t ld, double sign, const uint32_t *Xg, double *V, const gdca_chain_plan &c, double *sum_state,
                                unsigned char *x_state, int N, int sdim, int G, int t0, int t1)
{
    return chain_args{A, ld, sign, Xg, V, c.mask, c.thr, c.moves, sum_state, x_state, c.seed, c.stream0,
                      N, sdim, G, (c.flags & GDCA_SAMPLE_GAPS) != 0 ? 1 : 0, c.n_steps(), t0, t1};
}
