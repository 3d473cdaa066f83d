// Column histograms and theta = :auto  (compute_theta inside DCAUtils'
// compute_weighted_frequencies; reference call site src/GaussDCA.jl:28, doc README.md:78-80).
//
// The reference makes an all-pairs pass to get the mean pair identity.  The same integer
//   sum_{k<l} #{i : Z[i,k] == Z[i,l]}  =  sum_i sum_a c_ia (c_ia - 1) / 2
// follows from the per-column symbol counts c_ia, so this stage is one O(N*M) streaming
// pass (HBM-bound, N*M bytes) instead of M^2 N / 2 compares.  All integer, exact.
#include "gdca_internal.h"
#include "gdca_launch.h"

// ---- Z [M][N] -> Zt [N][M] and Zc [ceil(N/TJ)][M][TJ] in one pass (64 x 64 byte tiles through LDS) --------------------------
// The tile is read once -- one dword (four neighbouring columns) per lane where the rows are 4-byte aligned (N % 4 == 0 and an
// aligned Z), byte by byte otherwise: Z is the caller's pointer -- and leaves twice:
//   Zt: a thread transposes a 4 x 4 byte block in registers and stores one dword (four consecutive sequences) per column;
//   Zc: the TJ bytes of (column block, sequence) are contiguous in the tile's row: one 16-byte store per thread.
// Zc is what k_pair_tally stages from (zero padded up to the last column block; 16-byte aligned: the context's own buffer).
struct k_relayout_args {
    const int8_t *Z;
    int8_t *Zt;
    int8_t *Zc;
    int N;
    int M;
    int TJ;
};
static inline k_relayout_args k_relayout_mk(const int8_t *Z, int8_t *Zt, int8_t *Zc, int N, int M, int TJ)
{
    return k_relayout_args{Z, Zt, Zc, N, M, TJ};
}
template <int CAP>
__global__ __launch_bounds__(256) void k_relayout(const BatchArgs<k_relayout_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const int8_t *__restrict__ Z = a_.Z;
    int8_t *__restrict__ Zt = a_.Zt;
    int8_t *__restrict__ Zc = a_.Zc;
    int N = a_.N;
    int M = a_.M;
    int TJ = a_.TJ;
    __shared__ uint32_t tile[64][17];  // [sequence][four columns]; 17: the transposed reads below hit 64 different banks
    const int k0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int t = threadIdx.x;
    if (((N & 3) == 0) && ((reinterpret_cast<uintptr_t>(Z) & 3) == 0)) {
        const int d = t & 15, c = c0 + 4 * d;  // (N % 4 == 0: a dword is inside the row or outside it, never across its end)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kl = r * 16 + (t >> 4), k = k0 + kl;
            uint32_t v = 0;
            if (k < M && c < N) v = *reinterpret_cast<const uint32_t *>(Z + (size_t)k * N + c);
            tile[kl][d] = v;
        }
    } else {
        uint8_t *tb = reinterpret_cast<uint8_t *>(&tile[0][0]);
        const int tx = t & 63, ty = t >> 6;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kl = r * 4 + ty, k = k0 + kl, c = c0 + tx;
            tb[kl * 68 + tx] = (k < M && c < N) ? (uint8_t)Z[(size_t)k * N + c] : (uint8_t)0;
        }
    }
    __syncthreads();
    {  // Zc: 64 sequences x (64 / TJ) column blocks x (TJ / 16) 16-byte pieces = 256 stores, one per thread
        const int q16 = TJ >> 4;
        const int blk = t / (64 * q16), rem = t % (64 * q16);
        const int kl = rem / q16, h = rem % q16;
        const int k = k0 + kl, cb = c0 / TJ + blk;
        if (k < M && cb * TJ < N) {  // (column blocks past the last one that holds a column are not written)
            const int d0 = blk * (TJ >> 2) + 4 * h;
            const uint4 v = make_uint4(tile[kl][d0], tile[kl][d0 + 1], tile[kl][d0 + 2], tile[kl][d0 + 3]);
            *reinterpret_cast<uint4 *>(Zc + ((size_t)cb * M + k) * TJ + 16 * h) = v;
        }
    }
    {  // Zt: thread = (four sequences bk, four columns bc)
        const bool wide = ((M & 3) == 0) && ((reinterpret_cast<uintptr_t>(Zt) & 3) == 0);
        const int bk = t & 15, bc = t >> 4;
        uint32_t r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = tile[4 * bk + j][bc];
        const int k = k0 + 4 * bk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = c0 + 4 * bc + j;
            const uint32_t o = ((r[0] >> (8 * j)) & 255u) | (((r[1] >> (8 * j)) & 255u) << 8) | (((r[2] >> (8 * j)) & 255u) << 16) |
                               (((r[3] >> (8 * j)) & 255u) << 24);
            if (i < N && k < M) {
                int8_t *dst = Zt + (size_t)i * M + k;
                if (wide) {
                    *reinterpret_cast<uint32_t *>(dst) = o;  // (M % 4 == 0: k + 3 < M)
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < M) dst[e] = (int8_t)((o >> (8 * e)) & 255u);
                }
            }
        }
    }
}

void gdca_launch_relayout(hipStream_t s, const int8_t *Z, int8_t *Zt, int8_t *Zc, int N, int M, int TJ)
{
    dim3 grid((N + 63) / 64, (M + 63) / 64);
    (gdca_launch<k_relayout_args, k_relayout<1>, k_relayout<GDCA_MAXB>>(grid, dim3(256), 0, s, k_relayout_mk(Z, Zt, Zc, N, M, TJ)));
}

// ---- per-column symbol counts ---------------------------------------------------------------
// A workgroup owns a strip of 256 columns over a chunk of the sequences.  A wave reads one sequence's 256 bytes of the strip per
// instruction -- a dword, four neighbouring columns, per lane (byte loads where the rows are not 4-byte aligned) -- with
// HIST_ROWS sequences in flight, and counts into h[symbol][j][lane] in LDS: lane and j name the column, so the 64 lanes of an
// instruction hit 64 different banks whatever the symbols are, and the LDS adds (the workgroup's waves share the counters) return
// nothing the loop waits for.  Every counter of the output has ONE writer: chunk y's counts go to out + y * N * 32 with plain
// stores, and where the sequences are split k_column_hist_sum adds the chunks in a fixed order.  No global atomics, nothing to zero.
#define HIST_THREADS 1024  // (measured at N = 500, M = 50 000: 512 threads 17.1 us, 1024 14.2)
#define HIST_ROWS 8
struct k_column_hist_args {
    const int8_t *Z;
    uint32_t *out;
    int N;
    int M;
    int seq_per_block;
};
static inline k_column_hist_args k_column_hist_mk(const int8_t *Z, uint32_t *out, int N, int M, int seq_per_block)
{
    return k_column_hist_args{Z, out, N, M, seq_per_block};
}
template <int CAP>
__global__ __launch_bounds__(HIST_THREADS) void k_column_hist(const BatchArgs<k_column_hist_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const int8_t *__restrict__ Z = a_.Z;
    uint32_t *__restrict__ out = a_.out;
    int N = a_.N;
    int M = a_.M;
    int seq_per_block = a_.seq_per_block;
    constexpr int NW = HIST_THREADS / 64;
    static_assert(HIST_THREADS >= 512, "the store of the counts takes 512 threads");
    __shared__ __attribute__((aligned(16))) uint32_t h[32 * 256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int e = t; e < 32 * 256; e += HIST_THREADS) h[e] = 0;
    const int c = blockIdx.x * 256 + 4 * lane;
    const int nv = N - c < 4 ? N - c : 4;  // columns of this lane inside the alignment (<= 0: none)
    const int kbeg = blockIdx.y * seq_per_block;
    const int kend = min(M, kbeg + seq_per_block);
    const bool wide = ((N & 3) == 0) && ((reinterpret_cast<uintptr_t>(Z) & 3) == 0);  // (then nv is 4 or <= 0)
    __syncthreads();
    if (nv > 0) {
        for (int k = kbeg + wv; k < kend; k += NW * HIST_ROWS) {
            uint32_t v[HIST_ROWS];
#pragma unroll
            for (int u = 0; u < HIST_ROWS; ++u) {
                const int ku = k + u * NW;
                v[u] = 0;
                if (ku < kend) {
                    const int8_t *p = Z + (size_t)ku * N + c;
                    if (wide) {
                        v[u] = *reinterpret_cast<const uint32_t *>(p);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < nv) v[u] |= (uint32_t)(uint8_t)p[j] << (8 * j);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < HIST_ROWS; ++u) {
                if (k + u * NW < kend) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nv) atomicAdd(&h[((v[u] >> (8 * j)) & 31u) * 256 + j * 64 + lane], 1u);
                }
            }
        }
    }
    __syncthreads();
    {  // thread = (column, half of the symbols): 16 counters, 64 contiguous bytes of the output
        const int x = t & 255, half = t >> 8;
        const int l = x & 63, j = x >> 6;
        const int col = blockIdx.x * 256 + 4 * l + j;
        if (t < 512 && col < N) {
            uint32_t *dst = out + ((size_t)blockIdx.y * N + col) * 32 + 16 * half;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int z = 16 * half + 4 * g;
                const uint4 o = make_uint4(h[z * 256 + j * 64 + l], h[(z + 1) * 256 + j * 64 + l], h[(z + 2) * 256 + j * 64 + l],
                                           h[(z + 3) * 256 + j * 64 + l]);
                reinterpret_cast<uint4 *>(dst)[g] = o;
            }
        }
    }
}

struct k_column_hist_sum_args {
    const uint32_t *part;
    uint32_t *cnt;
    int total;
    int chunks;
};
static inline k_column_hist_sum_args k_column_hist_sum_mk(const uint32_t *part, uint32_t *cnt, int total, int chunks)
{
    return k_column_hist_sum_args{part, cnt, total, chunks};
}
template <int CAP>
__global__ __launch_bounds__(256) void k_column_hist_sum(const BatchArgs<k_column_hist_sum_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const uint32_t *__restrict__ part = a_.part;
    uint32_t *__restrict__ cnt = a_.cnt;
    int total = a_.total;
    int chunks = a_.chunks;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    uint32_t acc = 0;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(c + u) * total + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; c < chunks; ++c) acc += part[(size_t)c * total + e];
    cnt[e] = acc;
}

// chunks the sequences are split into: about one workgroup per compute unit, at least 64 sequences each
static int column_hist_split(int N, int M, int *spb_out)
{
    const int strips = (N + 255) / 256;
    int chunks = (256 + strips - 1) / strips;
    int spb = (M + chunks - 1) / chunks;
    if (spb < 64) spb = 64;
    chunks = (M + spb - 1) / spb;
    if (spb_out) *spb_out = spb;
    return chunks;
}

size_t gdca_column_hist_bytes(int N, int M)
{
    const int chunks = column_hist_split(N, M, nullptr);
    return (size_t)N * 32 * sizeof(uint32_t) * (size_t)(chunks > 1 ? 1 + chunks : 1);
}

void gdca_launch_column_hist(hipStream_t s, const int8_t *Z, uint32_t *cnt, int N, int M)
{
    int spb;
    const int chunks = column_hist_split(N, M, &spb);
    uint32_t *out = chunks > 1 ? cnt + (size_t)N * 32 : cnt;  // one chunk: its counts are the result
    (gdca_launch<k_column_hist_args, k_column_hist<1>, k_column_hist<GDCA_MAXB>>(dim3((N + 255) / 256, chunks), dim3(HIST_THREADS), 0, s, k_column_hist_mk(Z, out, N, M, spb)));
    if (chunks > 1)
        (gdca_launch<k_column_hist_sum_args, k_column_hist_sum<1>, k_column_hist_sum<GDCA_MAXB>>(dim3((N * 32 + 255) / 256, 1), dim3(256), 0, s, k_column_hist_sum_mk(out, cnt, N * 32, chunks)));
}

// ---- theta, threshold -------------------------------------------------------------------------
struct k_theta_finalize_args {
    const uint32_t *cnt;
    int N;
    int M;
    double theta_in;
    gdca_dev_scalars *sc;
};
static inline k_theta_finalize_args k_theta_finalize_mk(const uint32_t *cnt, int N, int M, double theta_in, gdca_dev_scalars *sc)
{
    return k_theta_finalize_args{cnt, N, M, theta_in, sc};
}
template <int CAP>
__global__ __launch_bounds__(256) void k_theta_finalize(const BatchArgs<k_theta_finalize_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const uint32_t *__restrict__ cnt = a_.cnt;
    int N = a_.N;
    int M = a_.M;
    double theta_in = a_.theta_in;
    gdca_dev_scalars *sc = a_.sc;
    __shared__ unsigned long long red[256];
    double theta = theta_in;
    if (theta_in < 0.0) {
        unsigned long long acc = 0;
        for (int e = threadIdx.x; e < N * 32; e += 256) {
            const unsigned long long c = cnt[e];
            acc += c * (c - 1) / 2;  // c == 0 -> 0 * (2^64-1) / 2 == 0
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const unsigned long long tot = red[0];
            sc->pair_sum = tot;
            if (M < 2) {
                theta = 0.0;
            } else {
                // same operation order as the oracle: tot / (N * (0.5 * M * (M - 1)))
                const double phi = (double)tot / ((double)N * (0.5 * (double)M * (double)(M - 1)));
                const double c = 0.38 * 0.32;
                const double t = c / phi;
                theta = t < 0.5 ? t : 0.5;
            }
        }
    } else if (threadIdx.x == 0) {
        sc->pair_sum = 0;
    }
    if (threadIdx.x == 0) {
        sc->theta = theta;
        sc->thresh = (int)floor(theta * (double)N);
    }
}

void gdca_launch_theta_finalize(hipStream_t s, const uint32_t *cnt, int N, int M, double theta_in,
                                gdca_dev_scalars *sc)
{
    (gdca_launch<k_theta_finalize_args, k_theta_finalize<1>, k_theta_finalize<GDCA_MAXB>>(dim3(1), dim3(256), 0, s, k_theta_finalize_mk(cnt, N, M, theta_in, sc)));
}

struct k_set_thresh_args {
    gdca_dev_scalars *sc;
    int thresh;
};
static inline k_set_thresh_args k_set_thresh_mk(gdca_dev_scalars *sc, int thresh)
{
    return k_set_thresh_args{sc, thresh};
}
template <int CAP>
__global__ void k_set_thresh(const BatchArgs<k_set_thresh_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    gdca_dev_scalars *sc = a_.sc;
    int thresh = a_.thresh;
    sc->thresh = thresh;
}

void gdca_launch_set_thresh(hipStream_t s, gdca_dev_scalars *sc, int thresh)
{
    (gdca_launch<k_set_thresh_args, k_set_thresh<1>, k_set_thresh<GDCA_MAXB>>(dim3(1), dim3(1), 0, s, k_set_thresh_mk(sc, thresh)));
}
