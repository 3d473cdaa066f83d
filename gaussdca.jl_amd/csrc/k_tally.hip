// Weighted one-/two-site frequency accumulation and the fused covariance build
// (DCAUtils compute_weighted_frequencies' accumulation, add_pseudocount, and the in-tree
// compute_C; reference call sites src/GaussDCA.jl:28, :30, :32/:76).
//
//   Pij[(i,a),(j,b)] = (1/Meff) sum_k W_k [Z[i,k]==a][Z[j,k]==b]          a,b in 1..s, s = q-1
//
// MI355X design.  This is a sparse tally (N(N+1)/2 * M weighted increments), not a GEMM: the
// dense one-hot product would be 400x more work.  A workgroup owns column i against a block
// of TJ = 32 columns j and keeps the 32 s x s histograms in LDS (100 KB at s = 20), laid out
// [a][b][j] so that a wave-instruction's 64 lanes (32 columns x 2 sequences) always touch 32
// different bank pairs whatever the symbols are.  Z is read in its natural layout: for one
// sequence the 32 bytes of the column block are contiguous.
//
// Accumulation is in 64-bit FIXED POINT (ds_add_u64): W_k is scaled by 2^shift with
// M * 2^shift <= 2^63, so the integer sums cannot overflow, are independent of the order in
// which waves reach the LDS atomics (bit-reproducible run to run), and resolve 2^-shift
// (7e-15 at M = 50k) -- finer than an f64 running sum of magnitude ~Meff/20.
//
// The epilogue applies 1/Meff, the pseudocount rule (diagonal blocks get pc/q on their
// diagonal only, off-diagonal blocks pc/q^2 everywhere) and subtracts Pi'Pi'^T, so the n x n
// covariance is written to HBM exactly once (8 n^2 bytes) and Pij never exists in memory.
#include "gdca_internal.h"
#include "gdca_launch.h"
#include <cstdlib>

typedef unsigned long long u64;

// ---- single-site sums and the sequences each column's pair tally visits: one kernel over Zt, one workgroup per column ------------
// Column i's M bytes are contiguous in Zt (k_relayout has just written them).  The row is walked in ALIGNED dwords -- four
// consecutive sequences per lane; where the row does not start on a dword (M % 4 != 0) the first and last dword reach into the
// neighbouring rows and those bytes are masked by their sequence index, so Zt needs 4-byte alignment and 3 bytes of slack.
//
// Pass one: Pifix[i][z] = sum_k Wfix[k] [Zt[i][k] & 31 == z] in u64, all 32 of them (bytes outside 1..q land where their low five
// bits say and raise GDCA_BAD_ALIGNMENT in sc->bad_symbol).  The sums are taken in bins[z][lane] in LDS: the lane index makes the 64 lanes of an
// ds_add_u64 conflict-free whatever the symbols are, the workgroup's waves share the bins, and nothing waits for an add.  The 64
// partial sums of a symbol are then added in a fixed order (integers: any order gives these bits) and stored -- one owner per sum.
//
// Pass two (TALLY_SKIP: keep != nullptr), from the same bytes, now in L2:
// sigma(i) = the symbol of column i with the largest single-site sum (1..q, ties to the smallest).  Only the sequences whose
// Z[i,k] is a legal symbol other than sigma(i) are tallied by k_pair_tally; row sigma(i) of every histogram is recovered afterwards
// from the column sums  sum_a H[a][b] = Pifix[j][b]  in u64 (exact: wrap-around cancels, the true value is < 2^63).  Those
// sequences are written in ascending order as  (k << 5) | Z[i,k]  into keep[i][0 .. keep_n[i]-1]: wave ballots place a kept
// sequence inside its wave, one wave scans the (slab, wave) counts of a step of PIK_THREADS * PIK_SLABS * 4 sequences.
#define PIK_THREADS 512  // (measured at N = 500, M = 50 000: 256 threads 52.7 us, 512 39.0, 1024 47.5)
#define PIK_SLABS 4
struct k_pi_keep_args {
    const int8_t *Zt;
    const u64 *Wfix;
    u64 *Pifix;
    uint32_t *keep;
    int *keep_n;
    uint8_t *sigma;
    int N;
    int M;
    int q;
    gdca_dev_scalars *sc;
};
static inline k_pi_keep_args k_pi_keep_mk(const int8_t *Zt, const u64 *Wfix, u64 *Pifix, uint32_t *keep, int *keep_n, uint8_t *sigma, int N, int M, int q, gdca_dev_scalars *sc)
{
    return k_pi_keep_args{Zt, Wfix, Pifix, keep, keep_n, sigma, N, M, q, sc};
}
template <int CAP>
__global__ __launch_bounds__(PIK_THREADS) void k_pi_keep(const BatchArgs<k_pi_keep_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const u64 *__restrict__ Wfix = a_.Wfix;
    u64 *__restrict__ Pifix = a_.Pifix;
    uint32_t *__restrict__ keep = a_.keep;
    int M = a_.M;
    int q = a_.q;
    gdca_dev_scalars *sc = a_.sc;
    constexpr int NW = PIK_THREADS / 64;
    constexpr int NC = PIK_SLABS * NW;  // (slab, wave) counts of one step, slab-major = ascending k
    static_assert(PIK_THREADS >= 256 && NC <= 64, "the fold below takes 256 threads; one wave scans the counts");
    __shared__ u64 bins[32 * 64];
    __shared__ u64 tot[32];
    __shared__ unsigned wcnt[2][NC], woff[2][NC + 1];
    const int i = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int8_t *zi = a_.Zt + (size_t)i * M;
    const int off = (int)(reinterpret_cast<uintptr_t>(zi) & 3);
    const uint32_t *__restrict__ zw = reinterpret_cast<const uint32_t *>(zi - off);  // dword d holds sequences 4 d - off .. + 3
    const int D = (off + M + 3) >> 2;
    const bool wpair = off == 0 && (reinterpret_cast<uintptr_t>(Wfix) & 15) == 0;  // four weights of a dword as two 16-byte loads
    for (int e = t; e < 32 * 64; e += PIK_THREADS) bins[e] = 0;
    __syncthreads();
    unsigned bad = 0;  // any byte outside 1..q
    for (int d0 = 0; d0 < D; d0 += PIK_THREADS * PIK_SLABS) {
        uint32_t z[PIK_SLABS];
        u64 w[PIK_SLABS][4];
#pragma unroll
        for (int u = 0; u < PIK_SLABS; ++u) {
            const int d = d0 + u * PIK_THREADS + t;
            const int k = 4 * d - off;
            z[u] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[u][j] = 0;
            if (d < D) {
                z[u] = zw[d];
                if (wpair && k + 3 < M) {
                    const ulonglong2 w0 = reinterpret_cast<const ulonglong2 *>(Wfix + k)[0];
                    const ulonglong2 w1 = reinterpret_cast<const ulonglong2 *>(Wfix + k)[1];
                    w[u][0] = w0.x;
                    w[u][1] = w0.y;
                    w[u][2] = w1.x;
                    w[u][3] = w1.y;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((unsigned)(k + j) < (unsigned)M) w[u][j] = Wfix[k + j];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PIK_SLABS; ++u) {
            const int d = d0 + u * PIK_THREADS + t;
            const int k = 4 * d - off;
            if (d < D) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((unsigned)(k + j) < (unsigned)M) {
                        const unsigned raw = (z[u] >> (8 * j)) & 255u;
                        bad |= (raw - 1u) >= (unsigned)q;
                        atomicAdd(&bins[(raw & 31u) * 64 + lane], w[u][j]);
                    }
                }
            }
        }
    }
    if (bad) atomicOr(&sc->bad_symbol, GDCA_BAD_ALIGNMENT);
    __syncthreads();
    if (t < 256) {  // eight threads fold the 64 partial sums of one symbol
        const int z = t >> 3, part = t & 7;
        u64 v = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) v += bins[z * 64 + part * 8 + e];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        if (part == 0) {
            tot[z] = v;
            Pifix[(size_t)i * 32 + z] = v;
        }
    }
    if (keep == nullptr) return;  // (uniform) the full loop needs no lists
    __syncthreads();
    unsigned sig = 1;
    u64 best = tot[1];
    for (int a = 2; a <= q; ++a) {
        const u64 v = tot[a];
        if (v > best) {
            best = v;
            sig = (unsigned)a;
        }
    }
    uint32_t *out = keep + (size_t)i * M;
    const u64 lt = (1ull << lane) - 1ull;
    unsigned base = 0;
    int par = 0;  // wcnt / woff are double-buffered by the step's parity: two barriers per step
    for (int d0 = 0; d0 < D; d0 += PIK_THREADS * PIK_SLABS, par ^= 1) {
        uint32_t z[PIK_SLABS];
        unsigned kpm[PIK_SLABS], pos[PIK_SLABS];
#pragma unroll
        for (int u = 0; u < PIK_SLABS; ++u) {
            const int d = d0 + u * PIK_THREADS + t;
            z[u] = d < D ? zw[d] : 0u;
        }
#pragma unroll
        for (int u = 0; u < PIK_SLABS; ++u) {
            const int d = d0 + u * PIK_THREADS + t;
            const int k = 4 * d - off;
            unsigned m = 0, pre = 0, cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned raw = (z[u] >> (8 * j)) & 255u;
                const bool kp = d < D && (unsigned)(k + j) < (unsigned)M && (raw - 1u) < (unsigned)q && raw != sig;
                const u64 bal = __ballot(kp);
                pre += (unsigned)__popcll(bal & lt);
                cnt += (unsigned)__popcll(bal);
                m |= (kp ? 1u : 0u) << j;
            }
            kpm[u] = m;
            pos[u] = pre;  // kept sequences of this slab in the lanes below this one
            if (lane == 0) wcnt[par][u * NW + wv] = cnt;
        }
        __syncthreads();
        if (wv == 0) {
            const unsigned v = lane < NC ? wcnt[par][lane] : 0u;
            unsigned incl = v;
#pragma unroll
            for (int o = 1; o < NC; o <<= 1) {
                const unsigned nb = __shfl_up(incl, o, 64);
                if (lane >= o) incl += nb;
            }
            if (lane < NC) woff[par][lane] = base + incl - v;
            if (lane == NC - 1) woff[par][NC] = base + incl;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PIK_SLABS; ++u) {
            if (kpm[u]) {
                const int k = 4 * (d0 + u * PIK_THREADS + t) - off;
                unsigned o = woff[par][u * NW + wv] + pos[u];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((kpm[u] >> j) & 1u) out[o++] = ((unsigned)(k + j) << 5) | ((z[u] >> (8 * j)) & 255u);
            }
        }
        base = woff[par][NC];
    }
    if (t == 0) {
        a_.keep_n[i] = (int)base;
        a_.sigma[i] = (uint8_t)sig;
    }
}

void gdca_launch_pi_keep(hipStream_t s, const int8_t *Zt, const u64 *Wfix, u64 *Pifix, uint32_t *keep, int *keep_n, uint8_t *sigma, int N, int M,
                         int q, gdca_dev_scalars *sc)
{
    (gdca_launch<k_pi_keep_args, k_pi_keep<1>, k_pi_keep<GDCA_MAXB>>(dim3(N, 1), dim3(PIK_THREADS), 0, s, k_pi_keep_mk(Zt, Wfix, Pifix, keep, keep_n, sigma, N, M, q, sc)));
}

struct k_pi_finalize_args {
    const u64 *Pifix;
    int N;
    int q;
    int fix_shift;
    const double *Meff_dev;
    double pc;
    double *Pi_true;
    double *Pi_pc;
    double *pi_max;
};
static inline k_pi_finalize_args k_pi_finalize_mk(const u64 *Pifix, int N, int q, int fix_shift, const double *Meff_dev, double pc, double *Pi_true, double *Pi_pc, double *pi_max)
{
    return k_pi_finalize_args{Pifix, N, q, fix_shift, Meff_dev, pc, Pi_true, Pi_pc, pi_max};
}
template <int CAP>
__global__ __launch_bounds__(256) void k_pi_finalize(const BatchArgs<k_pi_finalize_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const u64 *__restrict__ Pifix = a_.Pifix;
    int N = a_.N;
    int q = a_.q;
    int fix_shift = a_.fix_shift;
    const double *__restrict__ Meff_dev = a_.Meff_dev;
    double pc = a_.pc;
    double *__restrict__ Pi_true = a_.Pi_true;
    double *__restrict__ Pi_pc = a_.Pi_pc;
    double *__restrict__ pi_max = a_.pi_max;
    const int s = q - 1;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double mine = 0.0;
    if (e < N * s) {
        const int i = e / s, a = e % s;  // state a+1
        const double Meff = *Meff_dev;
        const double pt = ldexp((double)Pifix[(size_t)i * 32 + a + 1], -fix_shift) / Meff;
        if (Pi_true) Pi_true[e] = pt;
        mine = (1.0 - pc) * pt + pc / (double)q;
        if (Pi_pc) Pi_pc[e] = mine;
    }
    if (pi_max) {  // (uniform) the largest frequency with pseudocount: ||C||_1 <= 2 N pi_max, what k_cov_norm1 decides on
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine = fmax(mine, __shfl_xor(mine, o, 64));
        // non-negative doubles order like their bit patterns (*pi_max was zeroed with the run's scalars)
        if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<u64 *>(pi_max), (u64)__double_as_longlong(mine));
    }
}

// ||C||_1 of the covariance the pair tally has just written (full symmetric, ld) -- but only where it is NEEDED: the refinement
// screen of the fused path (gdca_inverse_outcome.h, gdca_cond_bound) is  cond_2(C) <= ||C||_1 q^2 / pc,  and  ||C||_1 <= 2 N pi_max  is at hand for
// nothing (a column of C sums, in absolute value, to at most  sum_j sum_b [Pij(jb, ia) + Pi(jb) Pi(ia)] <= 2 N Pi(ia)).  At the
// pseudocounts gDCA is used with that cheap bound already settles the question and every workgroup leaves at once; where it does
// not (pc = 0.2 with a conserved column; small pc), the columns are summed -- one pass over C before the sweep overwrites it.
struct k_cov_norm1_args {
    const double *C;
    size_t ld;
    int n;
    int N;
    int q;
    double pc;
    double cond_limit;
    gdca_dev_scalars *sc;
    int always;
};
static inline k_cov_norm1_args k_cov_norm1_mk(const double *C, size_t ld, int n, int N, int q, double pc, double cond_limit, gdca_dev_scalars *sc, int always)
{
    return k_cov_norm1_args{C, ld, n, N, q, pc, cond_limit, sc, always};
}
template <int CAP>
__global__ __launch_bounds__(256) void k_cov_norm1(const BatchArgs<k_cov_norm1_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const double *__restrict__ C = a_.C;
    size_t ld = a_.ld;
    int n = a_.n;
    int N = a_.N;
    int q = a_.q;
    double pc = a_.pc;
    double cond_limit = a_.cond_limit;
    gdca_dev_scalars *__restrict__ sc = a_.sc;
    int always = a_.always;
    const double cheap = pc > 0.0 ? 2.0 * (double)N * sc->pi_max * (double)q * (double)q / pc : HUGE_VAL;
    if (!always && cheap <= cond_limit) return;
    __shared__ double red[256];
    double best = 0.0;
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        double a = 0.0;
        for (int r = threadIdx.x; r < n; r += 256) a += fabs(C[(size_t)r + (size_t)c * ld]);
        red[threadIdx.x] = a;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        best = fmax(best, red[0]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<u64 *>(&sc->mat_norm1), (u64)__double_as_longlong(best));
}

void gdca_launch_cov_norm1(hipStream_t s, const double *C, size_t ld, int N, int q, double pc, double cond_limit, gdca_dev_scalars *sc, int always)
{
    (gdca_launch<k_cov_norm1_args, k_cov_norm1<1>, k_cov_norm1<GDCA_MAXB>>(dim3(512), dim3(256), 0, s, k_cov_norm1_mk(C, ld, N * (q - 1), N, q, pc, cond_limit, sc, always)));
}

void gdca_launch_pi_finalize(hipStream_t s, const u64 *Pifix, int N, int q, int fix_shift, const double *Meff_dev,
                             double pc, double *Pi_true, double *Pi_pc, double *pi_max)
{
    const int n = N * (q - 1);
    (gdca_launch<k_pi_finalize_args, k_pi_finalize<1>, k_pi_finalize<GDCA_MAXB>>(dim3((n + 255) / 256), dim3(256), 0, s, k_pi_finalize_mk(Pifix, N, q, fix_shift, Meff_dev, pc, Pi_true, Pi_pc, pi_max)));
}

// ---- pair tallies -----------------------------------------------------------------------------------
#define TALLY_THREADS 1024
#define TALLY_CHUNK 1024  // sequences staged per pass (one per thread)

// Workgroup = (column i) x (block of TJ columns j >= i's block), 1024 threads = 16 waves (the
// histograms take most of the LDS, so one or two workgroups per CU: the waves have to come from here).
// Per pass of 1024 sequences the block's TJ bytes of every sequence and a packed
// {row(Z[i,k]), Wfix[k]} word are staged in LDS (the next pass's global loads are in flight while
// the current one is tallied), then each wave walks 64 sequences, 64/TJ at a time: lane =
// (sequence, column j): one ds_read_u8 for Z[j,k], one broadcast ds_read_b64 for the packed word,
// one ds_add_u64 into hist[a][b][j].
//
// The histogram has s+2 columns per row (b = 0 and b = q are junk columns for padding / gaps) so
// the inner loop needs no validity test at all: an invalid Z[i,k] is staged as weight 0, lanes left
// of the diagonal tally into columns the epilogue never reads.
//
// SKIP (TALLY_SKIP, the default where it fits): the staged sequences of column i are k_pi_keep's list -- every sequence but
// those with Z[i,k] = sigma(i) or an illegal byte -- so at config C a pass of 1024 staged sequences is 1024 useful ones out of
// ~2400.  The histogram then has a row AND a column per symbol, [q][q][TJ] indexed by symbol - 1 (the gap's row takes the gap
// sequences, which the recovery needs; the gap's column also takes the zero padding and any illegal byte), and row sigma(i) is
// rebuilt in u64 after the last barrier: H[sigma][b] = Pifix[j][b] - sum_{a != sigma} H[a][b].  The integer tallies, and so
// every f64 value of the epilogue, are those of the full loop bit for bit.
struct k_pair_tally_args {
    const int8_t *Zc;
    const int8_t *Zt;
    const u64 *Wfix;
    int N;
    int M;
    int q;
    int fix_shift;
    const double *Meff_dev;
    double pc;
    const double *Pi_pc;
    int mode;
    double *out;
    size_t ld;
    const uint32_t *keep;   // SKIP: k_pi_keep's lists, keep_n, sigma; Pifix for the recovery
    const int *keep_n;
    const uint8_t *sigma;
    const u64 *Pifix;
};
static inline k_pair_tally_args k_pair_tally_mk(const int8_t *Zc, const int8_t *Zt, const u64 *Wfix, int N, int M, int q, int fix_shift, const double *Meff_dev, double pc, const double *Pi_pc, int mode, double *out, size_t ld,
                                                const uint32_t *keep, const int *keep_n, const uint8_t *sigma, const u64 *Pifix)
{
    return k_pair_tally_args{Zc, Zt, Wfix, N, M, q, fix_shift, Meff_dev, pc, Pi_pc, mode, out, ld, keep, keep_n, sigma, Pifix};
}
template <int CAP, int TJ, bool SKIP>
__global__ __launch_bounds__(TALLY_THREADS) void k_pair_tally(const BatchArgs<k_pair_tally_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const int8_t *__restrict__ Zc = a_.Zc;
    const int8_t *__restrict__ Zt = a_.Zt;
    const u64 *__restrict__ Wfix = a_.Wfix;
    int N = a_.N;
    int M = a_.M;
    int q = a_.q;
    int fix_shift = a_.fix_shift;
    const double *__restrict__ Meff_dev = a_.Meff_dev;
    double pc = a_.pc;
    const double *__restrict__ Pi_pc = a_.Pi_pc;
    int mode = a_.mode;
    double *__restrict__ out = a_.out;
    size_t ld = a_.ld;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = q - 1;
#ifdef GDCA_TALLY_OLD_MAP  // (measurement builds only: the rectangular grid with the skewed column block, empty workgroups left of the diagonal)
    const int i = blockIdx.y;
    const int jblk = (blockIdx.x + blockIdx.y) % gridDim.x;
    const int j0 = jblk * TJ;
    if (j0 + TJ - 1 < i) return;
#else
    // The grid is the member's working workgroups and nothing else (tally_grid), in one line: column block OUTERMOST, the widest
    // (last) first, row i fastest.  Column block jb pairs with rows 0 .. min(N, (jb + 1) TJ) - 1, so counted from the back the
    // blocks in front of jb hold TJ jb (jb + 1) / 2 ids: a closed form, inverted with a square root and corrected in integers.
    // Workgroups go to the 8 XCDs round-robin by linear id and a CU holds two, so the 512 resident at any time are consecutive rows
    // of the same one or two column blocks: every XCD's L2 is asked for the same 16 M bytes of Zc and the same Wfix, walked in the
    // same direction of k, and the rows -- whose kept lists are what makes a workgroup long or short -- are dealt round-robin.
    // (The rectangular grid it replaces, column block skewed by the row, had the 64 workgroups of an XCD on all 32 column blocks:
    // at N = 500, M = 50k its L2 hit rate was 37 % against 83 % now, and 7 564 of its 16 000 workgroups returned at once.)
    const unsigned lin = gridDim.x * gridDim.y - 1u - (blockIdx.y * gridDim.x + blockIdx.x);  // counted from the back: ascending (jb, i)
    const unsigned tri = lin / TJ;
    unsigned jb = (unsigned)((sqrtf(8.0f * (float)tri + 1.0f) - 1.0f) * 0.5f);
    while (jb * (jb + 1u) / 2u > tri) --jb;
    while ((jb + 1u) * (jb + 2u) / 2u <= tri) ++jb;  // (the last block may be narrow: its N rows are fewer ids than a full block's)
    const int jblk = (int)jb;
    const int j0 = jblk * TJ;
    const int i = (int)(lin - (unsigned)TJ * (jb * (jb + 1u) / 2u));
#endif

    const int NROW = SKIP ? q : s;                                                // histogram rows
    const int CB = SKIP ? 0 : 1;                                                  // histogram column of state b (0..s-1): b + CB
    const int RS = (SKIP ? q : s + 2) * TJ;                                       // u64 per histogram row a
    u64 *hist = reinterpret_cast<u64 *>(smem);                                    // [s][s+2][TJ]  (SKIP: [q][q][TJ])
    u64 *meta_s = hist + (size_t)NROW * RS;                                       // [TALLY_CHUNK]
    uint8_t *zs = reinterpret_cast<uint8_t *>(meta_s + TALLY_CHUNK);              // [TALLY_CHUNK][TJ]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int SPI = 64 / TJ;  // sequences per wave-instruction
    constexpr int NWAVE = TALLY_THREADS / 64;
    constexpr int SEQ_PER_WAVE = TALLY_CHUNK / NWAVE;  // 64
    constexpr int NV = TJ / 16;                        // dwordx4 loads per sequence
    static_assert(TALLY_CHUNK == TALLY_THREADS, "one staged sequence per thread");
    const int jl = lane % TJ, sub = lane / TJ;
    const u64 wmask = (1ull << 59) - 1;
    const unsigned qclamp = (unsigned)(SKIP ? q - 1 : s + 1);
    const int nk = SKIP ? a_.keep_n[i] : M;  // sequences to stage
    const uint32_t *__restrict__ keep_i = a_.keep + (size_t)i * M;

    for (int e = tid; e < NROW * RS; e += TALLY_THREADS) hist[e] = 0;

    // prefetch registers for one pass: this thread's sequence kc + tid.  The raw loads stay
    // untouched in registers until the LDS write of the NEXT pass, so a whole pass of tallies
    // covers their latency.  Plain scalars: an indexed uint4 array here goes to scratch.
    const int8_t *Zblk = Zc + (size_t)jblk * M * TJ;
    uint4 z0 = make_uint4(0, 0, 0, 0), z1 = z0;
    u64 wf = 0;
    int8_t av = 0;
    // SKIP: the list entry of the sequence TALLY_FETCH gathers next.  It is loaded a whole pass before that fetch (TALLY_ENTRY), so
    // the fetch issues its Zc and Wfix gathers from a register and no wave waits, right behind the staging barriers, for a load it
    // has only just issued.
    uint32_t en = 0;
#define TALLY_ENTRY(KC)                                                                       \
    do {                                                                                      \
        if (SKIP) {                                                                           \
            int k_ = (KC) + tid;                                                              \
            en = keep_i[k_ < nk ? k_ : nk - 1]; /* the same clamp as the fetch it feeds */    \
        }                                                                                     \
    } while (0)
#define TALLY_FETCH(KC)                                                                       \
    do {                                                                                      \
        int k_ = (KC) + tid;                                                                  \
        k_ = k_ < nk ? k_ : nk - 1; /* clamp: the tail is staged with weight 0 */             \
        if (SKIP) {                                                                           \
            av = (int8_t)(en & 31u);                                                          \
            k_ = (int)(en >> 5);                                                              \
        }                                                                                     \
        const uint4 *src_ = reinterpret_cast<const uint4 *>(Zblk + (size_t)k_ * TJ);          \
        z0 = src_[0];                                                                         \
        if (NV > 1) z1 = src_[1];                                                             \
        if (!SKIP) av = Zt[(size_t)i * M + k_];                                               \
        wf = Wfix[k_];                                                                        \
    } while (0)
    if (nk > 0) {  // (SKIP: an empty list stages nothing)
        TALLY_ENTRY(0);
        TALLY_FETCH(0);
        TALLY_ENTRY(TALLY_CHUNK);  // (unconditional, here and below: the clamp keeps it inside the list, and a load under a condition
                                   // of its own is waited for where it is issued)
    }
    for (int kc = 0; kc < nk; kc += TALLY_CHUNK) {
        __syncthreads();  // previous pass fully consumed (and hist zeroed, first time)
        {
            reinterpret_cast<uint4 *>(zs + (size_t)tid * TJ)[0] = z0;
            if (NV > 1) reinterpret_cast<uint4 *>(zs + (size_t)tid * TJ)[1] = z1;
            const unsigned a = (unsigned)(uint8_t)av - 1u;  // row index 0..s-1 when valid (SKIP: 0..q-1, the list holds legal symbols only)
            const bool valid = (SKIP || a < (unsigned)s) && (kc + tid < nk);
            meta_s[tid] = valid ? (((u64)a << 59) | (wf & wmask)) : 0ull;
        }
        __syncthreads();
        if (kc + TALLY_CHUNK < nk) {
            TALLY_FETCH(kc + TALLY_CHUNK);
            TALLY_ENTRY(kc + 2 * TALLY_CHUNK);
        }
        const int kw = wv * SEQ_PER_WAVE;
        // the last pass: a wave whose slice starts at or behind nk has nothing to add, one that straddles nk stops behind the step
        // of four instructions that covers it (the staged tail has weight 0: adds that feed nothing).  Wave-uniform, no barrier inside.
        const int left = nk - kc - __builtin_amdgcn_readfirstlane(kw);
        const int nit = left >= SEQ_PER_WAVE ? SEQ_PER_WAVE / SPI : left > 0 ? (left + 4 * SPI - 1) / (4 * SPI) * 4 : 0;
#pragma unroll 2
        for (int it = 0; it < nit; it += 4) {
            u64 m4[4];
            unsigned b4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = kw + (it + u) * SPI + sub;
                m4[u] = meta_s[kk];
                b4[u] = zs[kk * TJ + jl];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned a = (unsigned)(m4[u] >> 59);
                const unsigned b = min(b4[u] - (unsigned)(1 - CB), qclamp);  // (SKIP: symbol 0 wraps and lands in the gap's column)
                const unsigned idx = __umul24(a, (unsigned)RS) + __umul24(b, (unsigned)TJ) + (unsigned)jl;
                atomicAdd(&hist[idx], m4[u] & wmask);
            }
        }
    }
    __syncthreads();
#undef TALLY_FETCH

    // ---- SKIP: row sigma(i) from the column sums (the gap's row is never read: nothing to do where sigma(i) = q) ----
    if (SKIP) {
        const int sg = (int)a_.sigma[i] - 1;
        const u64 *__restrict__ Pifix = a_.Pifix;
        if (sg < s) {
            for (int e = tid; e < s * TJ; e += TALLY_THREADS) {
                const int b = e / TJ, l = e - b * TJ;
                const int jj = j0 + l;
                if (jj >= N || jj < i) continue;
                u64 v = Pifix[(size_t)jj * 32 + b + 1];
                for (int a = 0; a < q; ++a)
                    if (a != sg) v -= hist[(size_t)a * RS + b * TJ + l];
                hist[(size_t)sg * RS + b * TJ + l] = v;
            }
        }
    }

    // ---- epilogue: histograms -> Pij_true (mode 0) or covariance C (mode 1) ----
    // Pi' of column i and of the TJ columns of the block are staged in LDS first (the staging
    // area is free now): the per-element math then touches LDS and registers only.
    double *pi_i = reinterpret_cast<double *>(meta_s);  // [s]
    double *pi_j = pi_i + 32;                            // [TJ * s]
    if (mode == 1) {
        for (int e = tid; e < s; e += TALLY_THREADS) pi_i[e] = Pi_pc[i * s + e];
        for (int e = tid; e < TJ * s; e += TALLY_THREADS) {
            const int jj = j0 + e / s;
            pi_j[e] = (jj < N) ? Pi_pc[jj * s + (e % s)] : 0.0;
        }
    }
    __syncthreads();
    const double Meff = *Meff_dev;
    const double pcq = pc / (double)q;
    const double off_add = pcq / (double)q;
    const int total = s * s * TJ;
    // pass 1: element (row j*s+b, col i*s+a): contiguous over (j, b) for fixed a
    for (int e = tid; e < total; e += TALLY_THREADS) {
        const int a = e / (TJ * s), rem = e - a * (TJ * s);
        const int l = rem / s, b = rem - l * s;
        const int jj = j0 + l;
        if (jj >= N || jj < i) continue;
        const double pt = ldexp((double)hist[(size_t)a * RS + (b + CB) * TJ + l], -fix_shift) / Meff;
        double v = pt;
        if (mode == 1) {
            const double pij = (jj != i) ? ((1.0 - pc) * pt + off_add) : ((1.0 - pc) * pt + ((a == b) ? pcq : 0.0));
            v = pij - pi_i[a] * pi_j[rem];
        }
        out[(size_t)(jj * s + b) + (size_t)(i * s + a) * ld] = v;
    }
    // pass 2: the mirror element (row i*s+a, col j*s+b): contiguous over a for fixed (j, b)
    for (int e = tid; e < total; e += TALLY_THREADS) {
        const int l = e / (s * s), rem = e - l * (s * s);
        const int b = rem / s, a = rem - b * s;
        const int jj = j0 + l;
        if (jj >= N || jj <= i) continue;  // the diagonal block was written in full by pass 1
        const double pt = ldexp((double)hist[(size_t)a * RS + (b + CB) * TJ + l], -fix_shift) / Meff;
        double v = pt;
        if (mode == 1) {
            const double pij = (1.0 - pc) * pt + off_add;
            v = pij - pi_i[a] * pi_j[l * s + b];
        }
        out[(size_t)(i * s + a) + (size_t)(jj * s + b) * ld] = v;
    }
}

static size_t tally_lds_bytes(int s, int TJ, bool skip = false)
{
    const size_t hist = skip ? (size_t)(s + 1) * (s + 1) * TJ * 8 : (size_t)s * (s + 2) * TJ * 8;
    return hist + (size_t)TALLY_CHUNK * 8 + (size_t)TALLY_CHUNK * TJ;
}

// The workgroups of one family, in one line: column block jb against its rows 0 .. min(N, (jb + 1) TJ) - 1 (what k_pair_tally
// decodes).  The blocks in front of the last are full, so they hold TJ (1 + 2 + ... + (nblk - 1)) ids, and the last holds N.
static dim3 tally_grid(int N, int TJ)
{
#ifdef GDCA_TALLY_OLD_MAP
    return dim3((N + TJ - 1) / TJ, N);
#else
    const unsigned long long nblk = ((unsigned)N + TJ - 1) / TJ;
    return dim3((unsigned)((unsigned long long)TJ * (nblk * (nblk - 1) / 2) + (unsigned)N), 1);
#endif
}

int gdca_tally_tj(int q, int tj_wanted)
{
    // 16 columns per workgroup: 80 KB of histograms at s = 20, so TWO 1024-thread workgroups share a CU and one's staging
    // barriers and epilogue hide behind the other's atomics (measured at config C: 3.26 ms against 4.03 ms with 32 columns
    // and one workgroup per CU; the context option GDCA_TALLY_TJ=32 brings the wide form back for comparison)
    if (tj_wanted == 32 && tally_lds_bytes(q - 1, 32) <= 160 * 1024) return 32;
    return 16;
}

bool gdca_tally_skip(int q, int TJ, int skip_wanted, int M)
{
    // the [q][q][TJ] histograms must leave as many workgroups per CU as the full loop's [s][s+2][TJ] (q = 21, TJ = 16: 81 024 B
    // against 80 896, two per CU either way); the list entries hold k in 27 bits
    const size_t lds = 160 * 1024, full = tally_lds_bytes(q - 1, TJ), skip = tally_lds_bytes(q - 1, TJ, true);
    return skip_wanted && M <= (1 << 27) && skip <= lds && lds / skip >= lds / full;
}

void gdca_launch_pair_tally(hipStream_t st, const int8_t *Zc, const int8_t *Zt, const u64 *Wfix, int N, int M, int q,
                            int fix_shift, const double *Meff_dev, double pc, const double *Pi_pc, int mode,
                            double *out, size_t ld, int TJ, const uint32_t *keep, const int *keep_n, const uint8_t *sigma,
                            const u64 *Pifix)
{
    const int s = q - 1;
    const bool skip = keep != nullptr;
    const k_pair_tally_args a = k_pair_tally_mk(Zc, Zt, Wfix, N, M, q, fix_shift, Meff_dev, pc, Pi_pc, mode, out, ld, keep, keep_n, sigma, Pifix);
    const size_t lds = tally_lds_bytes(s, TJ, skip);
    const dim3 grid = tally_grid(N, TJ);
    if (TJ == 32) {
        if (skip)
            (gdca_launch<k_pair_tally_args, k_pair_tally<1, 32, true>, k_pair_tally<GDCA_MAXB, 32, true>>(grid, dim3(TALLY_THREADS), lds, st, a));
        else
            (gdca_launch<k_pair_tally_args, k_pair_tally<1, 32, false>, k_pair_tally<GDCA_MAXB, 32, false>>(grid, dim3(TALLY_THREADS), lds, st, a));
    } else {
        if (skip)
            (gdca_launch<k_pair_tally_args, k_pair_tally<1, 16, true>, k_pair_tally<GDCA_MAXB, 16, true>>(grid, dim3(TALLY_THREADS), lds, st, a));
        else
            (gdca_launch<k_pair_tally_args, k_pair_tally<1, 16, false>, k_pair_tally<GDCA_MAXB, 16, false>>(grid, dim3(TALLY_THREADS), lds, st, a));
    }
}

// ---- the covariance of one pseudocount from stored tallies (gdca_run_multi) ---------------------------------------------------------
// Pij_true (n x n, full symmetric, ld = n: what k_pair_tally's mode 0 wrote) and Pi' of this pseudocount (k_pi_finalize) -> C in the
// inverse's buffer (ld = n_pad), both triangles.  Every element is k_pair_tally's epilogue expression (pass 1) copied verbatim, with
// the same operands -- Pij_true there is this very f64 value before it is stored -- so under -ffp-contract=off the two builds agree
// bit for bit.  (A shared inline helper was tried: it moves k_pair_tally's register allocation, so the epilogue is left as it was.)
// HBM-bound: 8 n^2 bytes read, 8 n^2 written.  A workgroup owns one column and ROWS_PER_THREAD x 256 rows of it: lanes walk the rows, so
// the reads of Pij_true and Pi' and the writes of C are all contiguous along a column.
#define COV_ROWS_PER_THREAD 4
struct k_cov_from_pij_args {
    const double *Pij;
    const double *Pi_pc;
    int n;
    int q;
    double pc;
    double *out;
    size_t ld;
    size_t ldp;  // leading dimension of Pij: n, or -- a principal block of whole sites (the marginal fits of the log-odds) -- the joint n
};
static inline k_cov_from_pij_args k_cov_from_pij_mk(const double *Pij, const double *Pi_pc, int n, int q, double pc, double *out, size_t ld,
                                                    size_t ldp)
{
    return k_cov_from_pij_args{Pij, Pi_pc, n, q, pc, out, ld, ldp};
}
template <int CAP>
__global__ __launch_bounds__(256) void k_cov_from_pij(const BatchArgs<k_cov_from_pij_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const double *__restrict__ Pij = a_.Pij;
    const double *__restrict__ Pi_pc = a_.Pi_pc;
    int n = a_.n;
    int q = a_.q;
    double pc = a_.pc;
    double *__restrict__ out = a_.out;
    size_t ld = a_.ld;
    const int s = q - 1;
    const int c = blockIdx.y;
    const int ic = c / s;
    const double pcq = pc / (double)q;
    const double off_add = pcq / (double)q;
    const double pi_c = Pi_pc[c];
    const double *__restrict__ src = Pij + (size_t)c * a_.ldp;
    double *__restrict__ dst = out + (size_t)c * ld;
    const int r0 = blockIdx.x * (256 * COV_ROWS_PER_THREAD) + threadIdx.x;
    double pt[COV_ROWS_PER_THREAD], pr[COV_ROWS_PER_THREAD];
#pragma unroll
    for (int u = 0; u < COV_ROWS_PER_THREAD; ++u) {  // all loads first: COV_ROWS_PER_THREAD of each in flight
        const int r = r0 + u * 256;
        pt[u] = r < n ? src[r] : 0.0;
        pr[u] = r < n ? Pi_pc[r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < COV_ROWS_PER_THREAD; ++u) {
        const int r = r0 + u * 256;
        if (r >= n) continue;
        const int jj = r / s, i = ic;  // row site, column site: the names of k_pair_tally's pass 1
        const bool ab = r == c;        // (a == b) inside the diagonal block
        const double pij = (jj != i) ? ((1.0 - pc) * pt[u] + off_add) : ((1.0 - pc) * pt[u] + (ab ? pcq : 0.0));
        dst[r] = pij - pi_c * pr[u];
    }
}

// ldp != 0: the principal block of N whole sites whose first element Pij and Pi_pc point at, inside a Pij of leading dimension ldp -- an
// element depends on its row and column only through their difference of sites and their equality, so the block's entries are bit for
// bit the entries of the joint covariance
void gdca_launch_cov_from_pij(hipStream_t s, const double *Pij, const double *Pi_pc, int N, int q, double pc, double *out, size_t ld, size_t ldp)
{
    const int n = N * (q - 1);
    const int rows = 256 * COV_ROWS_PER_THREAD;
    (gdca_launch<k_cov_from_pij_args, k_cov_from_pij<1>, k_cov_from_pij<GDCA_MAXB>>(dim3((n + rows - 1) / rows, n), dim3(256), 0, s, k_cov_from_pij_mk(Pij, Pi_pc, n, q, pc, out, ld, ldp ? ldp : (size_t)n)));
}
