// All-pairs Hamming reweighting (compute_weights inside DCAUtils' compute_weighted_frequencies; reference call site
// src/GaussDCA.jl:28): a LOWER BOUND of every pair's distance on the fp4 matrix pipe -- the CONSENSUS bound.
//
// Only pairs below the threshold count, so any cheap quantity that is never larger than the distance sorts the pairs: what passes
// goes to k_hamming_refine (k_hamming.hip), which counts exactly from the alignment's bytes -- the neighbour counts are the same
// integers whatever bound made the list.
//
// The bound.  sigma(i) = the most frequent symbol of column i (the argmax of the column histogram, ties to the smallest symbol), and
// x_k(i) = [Z[k, i] != sigma(i)].  Where exactly one of two sequences carries sigma(i) the two differ, so
//     D1(k, l) = popcount(x_k xor x_l) <= d(k, l),
// and D1 counts POSITIONS.  (Round 6's first bound on this pipe counted the differing BITS of the three low planes, D / 3 <= d: it
// kept 0.52 of d and listed 56 % of all pairs of the benchmark family, whose typical pair sits at d = 0.65 N with the threshold at
// 0.35 N; measured, never chosen, replaced by this one.  D1 keeps 0.75 of d there -- median 244 of 325 at N = 500 -- and lists 9.3e-4
// of the pairs against 1.85e-4 true neighbours and 2.4e-4 for the three-plane bound of k_hamming<3>; tools/hamming_alive.py
// --bound consensus reproduces the figures on the CPU.)  Any sigma gives a valid bound -- it only has to be the same for both
// operands, and deterministic, so that the list is reproducible.
// D1 is a Gram matrix: with x coded as the fp4 number (+1.0, -1.0)[x], S = sum over the N positions of a * b = N - 2 D1.
// v_mfma_scale_f32_32x32x64_f8f6f4 with both operands E2M1 multiplies 32 x 32 x 64 of them per instruction, exactly (|S| <= N in f32
// accumulators): M^2 / 2 x 32 NW MACs, 6.4e11 at config C, where the three-plane loop issues 6.25e11 x 4 / 32 VALU instructions.
//
// Layout.  k_fp4_image writes a row-major image of nibbles straight from the alignment's bytes: row = sequence, one 16-byte entry
// per 32-position word, entries padded to whole LDS chunks (eight) and rows to a multiple of 256.  Nibble = +1.0 where Z = sigma,
// -1.0 where not; positions beyond N, pad entries and rows beyond M are 0.0 nibbles, which add nothing to S -- so K, the number of
// terms of S that are +-1, is N for every pair of real sequences, and a row of 0.0 has S = 0 (it is kept out by its index, not by S).
// One k step of the MFMA is 64 nibbles = two entries; a lane holds row (lane % 32) and entry (lane / 32) of the step for A and for
// B alike -- the sum over k does not care in which order the nibbles sit inside a lane as long as both operands use the same, and
// both come from the same image.
// k_hamming_fp4: a 1024-thread workgroup (16 waves of 64 x 64 = 2 x 2 MFMA blocks) walks up to F4_SEG consecutive 256 x 256 tiles
// J of ONE tile row I of the upper triangle.  Operands are staged global -> registers -> LDS in chunks of four k steps; the stream
// of chunks runs across the tiles of the walk, double-buffered, one barrier per chunk, so only the first chunk of a walk is waited
// for with nothing to do.  Where a row strip is at most two chunks (N <= 512) the A strip is loaded once and stays in LDS for the
// whole walk (ARES).  Rows of the triangle are cut into walks of F4_SEG tiles, all about equally long, which balances the triangle.
// The epilogue, per tile, compares S with N - 2 thresh.  Shader-clock stamps (-DGDCA_F4_STAMPS, tools/fp4_stamps.py,
// profiles/fp4_feed_stamps_C.txt) showed that it, not the loads, was 61 % of a tile's 16 200 clocks at C (the wait for the loads:
// 4 %): its scan ran 64 compares with their validity tests in every wave that held a single candidate, then two barriers and the
// wait for a device-wide atomic.  Now: one maximum per four accumulators and a wave-uniform branch, the validity tests only behind
// a mask that is not empty; a wave's candidates go, by a prefix sum and one LDS atomic, to the tile's LDS list (two lists, tile
// parity); the chunk's own barrier publishes it, and wave 0 flushes it to the global list under the NEXT chunk -- the one
// device-wide atomic per tile is issued before that chunk's MFMAs and waited for behind them.  What a tile holds beyond its LDS list
// goes straight to the global list with an atomic per wave.  The listed set is the same; its order is not.
#include <algorithm>

#include "gdca_internal.h"
#include "gdca_launch.h"

typedef int fp4x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#define F4_TILE 256          // sequences per side of a pair tile
#define F4_KC 4              // k steps (of 64 nibbles = 32 bytes per row) per LDS chunk
#define F4_ROW (F4_KC * 32 + 16)  // bytes per row of a chunk in LDS: 128 + a 16-byte pad (16-byte reads of 32 rows: no bank is hit twice in a phase)
#define F4_OP (F4_TILE * F4_ROW)  // one operand's chunk
#define F4_LDS (4 * F4_OP)        // A (two chunks: resident, or two buffers) and B (two buffers): 147 456 bytes
#define F4_SEG 8             // tiles of one row a workgroup walks

// entries per row of the image: the NW real ones, padded with 0.0 nibbles (which add nothing to S) to whole LDS chunks of 2 F4_KC
static inline int f4_entries(int NW) { return (NW + 2 * F4_KC - 1) / (2 * F4_KC) * (2 * F4_KC); }
static inline size_t f4_image_only_bytes(int N, int M)
{
    const size_t NW = (size_t)(N + 31) / 32, rows = ((size_t)M + F4_TILE - 1) / F4_TILE * F4_TILE;
    return rows * (size_t)f4_entries((int)NW) * 16;
}
// the image, and behind it sigma: one byte per position of the padded row (32 per entry)
size_t gdca_fp4_image_bytes(int N, int M)
{
    return f4_image_only_bytes(N, M) + (size_t)f4_entries((N + 31) / 32) * 32;
}

// 8 bits -> 8 nibbles (0x2 | bit << 3: +1.0 / -1.0 in E2M1), bit i in nibble i; nibbles whose bit of `valid` is clear: 0.0
__device__ __forceinline__ uint32_t f4_spread8(uint32_t b)
{
    uint32_t x = b & 0xffu;
    x = (x | (x << 12)) & 0x000f000fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x;
}
__device__ __forceinline__ uint32_t f4_nibbles8(uint32_t differs, uint32_t valid)
{
    return ((f4_spread8(differs) << 3) | 0x22222222u) & (f4_spread8(valid) * 0xfu);
}
// the sign bits of 8 nibbles -> 8 bits (the inverse of f4_spread8 on bit 3 of every nibble)
__device__ __forceinline__ uint32_t f4_signs8(uint32_t v)
{
    uint32_t x = (v >> 3) & 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000f000fu;
    x = (x | (x >> 12)) & 0xffu;
    return x;
}

// ---- sigma: the most frequent symbol of every column ------------------------------------------------------------------------------
struct k_fp4_sigma_args {
    const uint32_t *hist;  // [N][32] counts of (byte & 31) (k_column_hist)
    uint8_t *sigma;        // [32 E]: positions beyond N: 0
    int N, NP;             // NP = 32 E
};
template <int CAP>
__global__ __launch_bounds__(256) void k_fp4_sigma(const BatchArgs<k_fp4_sigma_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const uint32_t *__restrict__ hist = a_.hist;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a_.NP) return;
    uint32_t best = 0u, bz = 0u;
    if (i < a_.N) {
        const uint4 *h = reinterpret_cast<const uint4 *>(hist + (size_t)i * 32);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const uint4 v = h[g];
            const uint32_t c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c[j] > best) {  // (strict: a tie stays with the smaller symbol)
                    best = c[j];
                    bz = (uint32_t)(4 * g + j);
                }
        }
    }
    a_.sigma[i] = (uint8_t)bz;
}

// ---- the fp4 image of the consensus plane ---------------------------------------------------------------------------------------------
// thread <-> (sequence, word), words fastest: the threads of a row read its bytes and write its entries side by side
struct k_fp4_image_args {
    const int8_t *Z;       // [M][N]
    const uint8_t *sigma;  // [32 E]
    uint4 *img;            // [rows][E] x 16 bytes
    int N, M, E, rows;
};
template <int CAP>
__global__ __launch_bounds__(256) void k_fp4_image(const BatchArgs<k_fp4_image_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const int8_t *__restrict__ Z = a_.Z;
    const uint8_t *__restrict__ sigma = a_.sigma;
    uint4 *__restrict__ img = a_.img;
    const int N = a_.N, M = a_.M, E = a_.E;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)a_.rows * E) return;
    const int k = (int)(g / E), w = (int)(g - (long long)k * E);
    uint32_t diff = 0u, valid = 0u;  // bit b: position 32 w + b differs from sigma / is a position of the alignment
    const int nb = min(32, N - w * 32);  // (<= 0: a pad entry)
    if (k < M && nb > 0) {
        const int8_t *src = Z + (size_t)k * N + (size_t)w * 32;
        valid = nb == 32 ? 0xffffffffu : ((1u << nb) - 1u);
        if (nb == 32 && (N & 3) == 0 && (reinterpret_cast<uintptr_t>(Z) & 3) == 0) {
            const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src), *g4 = reinterpret_cast<const uint32_t *>(sigma + w * 32);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t x = (s4[j] & 0x1f1f1f1fu) ^ g4[j];  // bytes that differ -> one bit each
                x |= x >> 4;
                x |= x >> 2;
                x |= x >> 1;
                x &= 0x01010101u;
                diff |= (((x * 0x01020408u) >> 24) & 0xfu) << (4 * j);
            }
        } else {
            for (int b = 0; b < nb; ++b) diff |= (uint32_t)(((uint32_t)(uint8_t)src[b] & 31u) != (uint32_t)sigma[w * 32 + b]) << b;
        }
    }
    // (rows beyond the alignment and pad entries: valid = 0, all 0.0)
    img[g] = make_uint4(f4_nibbles8(diff, valid), f4_nibbles8(diff >> 8, valid >> 8), f4_nibbles8(diff >> 16, valid >> 16), f4_nibbles8(diff >> 24, valid >> 24));
}

// ---- S = X X^T by 256 x 256 tiles, thresholded ---------------------------------------------------------------------------------------
__device__ __forceinline__ void f4_tri_decode(int t, int Mt, int &I, int &J)
{
    // t in [0, Mt (Mt + 1) / 2) -> (I, J), I <= J, row-major over the upper triangle
    const double b = 2.0 * Mt + 1.0;
    int i = (int)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    i = max(0, min(i, Mt - 1));
    auto start = [Mt](int r) { return (long long)r * Mt - (long long)r * (r - 1) / 2; };
    while (i > 0 && start(i) > t) --i;
    while (i < Mt - 1 && start(i + 1) <= t) ++i;
    I = i;
    J = i + (int)(t - start(i));
}

struct k_hamming_fp4_args {
    const unsigned char *img;  // the image, E entries of 16 bytes per row
    int E, M, Mt, N;           // Mt: 256-tiles per side
    gdca_dev_scalars *sc;
    int2 *cand_list;
    unsigned cand_cap;
};
// A tile's candidates wait in LDS, behind the operands, for the chunk after the tile: two lists (tile t of a walk: list t % 2) of
// F4_LCAP packed entries (row of the tile << 8 | column of the tile) and their two counters
#define F4_LCAP 1536
#define F4_LDS_ALL (F4_LDS + 2 * F4_LCAP * 4 + 16)  // 159 760 bytes of the 160 KB a workgroup may have

#ifdef GDCA_F4_STAMPS
// tools/fp4_stamps.py only: shader-clock stamps of one lane of eight workgroups (walk 1 of the tile rows 0, 16, .., 112),
// [workgroup][chunk of the walk][phase]; phases: 0 top of the chunk, 1 after its MFMAs, 2 after the LDS stores, 3 / 4 the
// epilogue's begin and end (last chunk of a tile; else 0), 5 behind the chunk's barrier, 6 / 7 begin and end of the flush of the
// tile before (first chunk of a tile; else 0), 8 the epilogue's scan done, 9 the wave's run of the list taken (0: no candidate)
#define F4_STAMP_WG 8
#define F4_STAMP_IT 32
#define F4_STAMP_PH 10
__device__ long long g_f4_stamps[F4_STAMP_WG * F4_STAMP_IT * F4_STAMP_PH];
extern "C" int gdca_fp4_stamps(long long *out, int clear)
{
    if (clear) {
        static long long zero[F4_STAMP_WG * F4_STAMP_IT * F4_STAMP_PH];
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_f4_stamps), zero, sizeof(zero));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_f4_stamps), sizeof(g_f4_stamps));
}
#define F4_STAMP(it, ph)                                                                                                  \
    do {                                                                                                                  \
        if (f4_stamped && tid == 0 && (it) < F4_STAMP_IT)                                                                 \
            g_f4_stamps[(((int)blockIdx.y >> 4) * F4_STAMP_IT + (it)) * F4_STAMP_PH + (ph)] = (long long)clock64();       \
    } while (0)
#else
#define F4_STAMP(it, ph) do { } while (0)
#endif
// ARES: the A strip (at most two chunks) is loaded once and stays in LDS; else A is streamed beside B
template <int CAP, bool ARES>
__global__ __launch_bounds__(1024) void k_hamming_fp4(const BatchArgs<k_hamming_fp4_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    gdca_dev_scalars *__restrict__ sc = a_.sc;
    if (sc->ham_mode != 2) return;
    const int thresh = sc->thresh;
    if (thresh <= 0) return;  // theta == 0: every n_k = 1
    const unsigned char *__restrict__ img = a_.img;
    const int E = a_.E, M = a_.M, Mt = a_.Mt;
    int2 *__restrict__ cand_list = a_.cand_list;
    const unsigned cand_cap = a_.cand_cap;
    extern __shared__ __attribute__((aligned(16))) unsigned char f4_lds[];

    // the walk: tiles J0 .. J1 - 1 of row I (grid: x = walk of the row, y = row; rows near the bottom of the triangle have fewer walks)
    const int I = (int)blockIdx.y, J0 = I + (int)blockIdx.x * F4_SEG;
    if (J0 >= Mt) return;
    const int J1 = min(Mt, J0 + F4_SEG);
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wv & 3, wc = wv >> 2;  // (wv: on the scalar side)
    const int l32 = lane & 31, lh = lane >> 5;
#ifdef GDCA_F4_STAMPS
    const bool f4_stamped = blockIdx.x == 1 && (blockIdx.y & 15) == 0 && (blockIdx.y >> 4) < F4_STAMP_WG && blockIdx.z == 0;
#endif
    unsigned *const f4_list = reinterpret_cast<unsigned *>(f4_lds + F4_LDS), *const f4_cnt = f4_list + 2 * F4_LCAP;
    if (tid == 0) {
        f4_cnt[0] = 0u;
        f4_cnt[1] = 0u;
    }
    const size_t rowbytes = (size_t)E * 16;
    const int nchunk = E / (2 * F4_KC);  // (rows hold whole chunks; ARES: 1 or 2)
    const int total = (J1 - J0) * nchunk;  // chunks of the walk

    // staging: a chunk is 256 rows x 8 pieces of 16 bytes per operand; thread t takes pieces t and t + 1024 of either: piece id -> row
    // id / 8, piece id % 8 (eight consecutive threads: 128 contiguous bytes of a row).  Named registers: as an array behind lambdas
    // the pieces lived in scratch.  LDS: regions 0, 1 = A (ARES: chunks 0, 1 of the strip; else two buffers), 2, 3 = B's two buffers.
    const int srow = tid >> 3, spc = tid & 7;  // (pieces t and t + 1024: rows srow and srow + 128)
    // (a lane's place inside a tile's rows as a 32-bit offset: the tile's and the chunk's address stay on the scalar side)
    const unsigned goff = (unsigned)srow * (unsigned)rowbytes + (unsigned)spc * 16u;
    const size_t half = (size_t)128 * rowbytes, tilebytes = (size_t)F4_TILE * rowbytes;
    const unsigned char *const ga = img + (size_t)I * tilebytes;
    unsigned char *la = f4_lds + srow * F4_ROW + spc * 16;
    uint4 s0, s1, s2, s3;
    s0 = s1 = make_uint4(0u, 0u, 0u, 0u);
#define F4_LOAD_A(ch)                                                                     \
    do {                                                                                  \
        const unsigned char *g_ = ga + (size_t)(ch) * (32 * F4_KC);                       \
        s0 = *reinterpret_cast<const uint4 *>(g_ + goff);                                 \
        s1 = *reinterpret_cast<const uint4 *>(g_ + half + goff);                          \
    } while (0)
#define F4_LOAD_B(J, ch)                                                                                      \
    do {                                                                                                      \
        const unsigned char *g_ = img + (size_t)(J) * tilebytes + (size_t)(ch) * (32 * F4_KC);                \
        s2 = *reinterpret_cast<const uint4 *>(g_ + goff);                                                     \
        s3 = *reinterpret_cast<const uint4 *>(g_ + half + goff);                                              \
    } while (0)
#define F4_STORE_A(region)                                                                \
    do {                                                                                  \
        unsigned char *d_ = la + (size_t)(region) * F4_OP;                                \
        *reinterpret_cast<uint4 *>(d_) = s0;                                              \
        *reinterpret_cast<uint4 *>(d_ + 128 * F4_ROW) = s1;                               \
    } while (0)
#define F4_STORE_B(buf)                                                                   \
    do {                                                                                  \
        unsigned char *d_ = la + (size_t)(2 + (buf)) * F4_OP;                             \
        *reinterpret_cast<uint4 *>(d_) = s2;                                              \
        *reinterpret_cast<uint4 *>(d_ + 128 * F4_ROW) = s3;                               \
    } while (0)

    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int one = 0x7f7f7f7f;  // E8M0 scale 2^0 for both operands

    // this lane's rows of the two operands inside a chunk: row (lane % 32) of its wave's first block, entry (lane / 32) of a k step
    const unsigned char *abase = f4_lds + (wr * 64 + l32) * F4_ROW + lh * 16, *bbase = f4_lds + 2 * F4_OP + (wc * 64 + l32) * F4_ROW + lh * 16;
    // candidates: S > N - 2 thresh  <=>  D1 = (N - S) / 2 < thresh.  (K = N: the positions beyond N are 0.0 nibbles in both operands.)
    const float limit = (float)(a_.N - 2 * thresh);

    if constexpr (ARES) {
        F4_LOAD_A(0);
        F4_STORE_A(0);
        if (nchunk > 1) {
            F4_LOAD_A(1);
            F4_STORE_A(1);
        }
    } else {
        F4_LOAD_A(0);
        F4_STORE_A(0);
    }
    F4_LOAD_B(J0, 0);
    F4_STORE_B(0);
    __syncthreads();
    // The flush of a tile's LDS list to the global list (wave 0; n > 0 entries of list q, tile Jt; b64: what lane 0's device-wide atomic
    // returned -- beyond the capacity nothing is written)
#define F4_FLUSH_WRITE(q, Jt, n, b64)                                                                                          \
    do {                                                                                                                       \
        const unsigned lo_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((b64) & 0xffffffffull));                 \
        const unsigned hi_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((b64) >> 32));                           \
        const unsigned base_ = (hi_ != 0u || lo_ > cand_cap) ? cand_cap : lo_;                                                 \
        const unsigned *lst_ = f4_list + (q) * F4_LCAP;                                                                        \
        for (unsigned k_ = (unsigned)lane; k_ < (n); k_ += 64u) {                                                              \
            const unsigned e_ = lst_[k_], slot_ = base_ + k_;                                                                  \
            if (slot_ < cand_cap) cand_list[slot_] = make_int2(I * F4_TILE + (int)(e_ >> 8), (Jt) * F4_TILE + (int)(e_ & 255u)); \
        }                                                                                                                      \
    } while (0)
    unsigned fl_n = 0u;               // wave 0: entries of the tile before in its LDS list, their place in the global list asked for
    unsigned long long fl_base = 0ull;  // (lane 0) and not yet waited for
    int J = J0, ch = 0;  // the chunk being multiplied
    for (int it = 0; it < total; ++it) {
        const int buf = it & 1;
        const bool more = it + 1 < total;
        const bool last = ch + 1 == nchunk;  // (of tile J)
        const int Jn = last ? J + 1 : J, chn = last ? 0 : ch + 1;
        F4_STAMP(it, 0);
        if (more) {  // in flight under this chunk's MFMAs
            if constexpr (!ARES) F4_LOAD_A(chn);
            F4_LOAD_B(Jn, chn);
        }
        if (wv == 0 && ch == 0 && it > 0) {
            // the tile before is complete and the barrier behind it has published its list: ONE device-wide atomic asks for its place
            // in the global list now; the answer is waited for behind this chunk's MFMAs.  The counter starts over: its next adds
            // are the tile after this one's, behind this chunk's barrier.
            const int q = (J - 1 - J0) & 1;
            fl_n = min((unsigned)__builtin_amdgcn_readfirstlane((int)f4_cnt[q]), (unsigned)F4_LCAP);  // (on the scalar side)
            if (lane == 0) {
                f4_cnt[q] = 0u;
                if (fl_n) fl_base = atomicAdd(&sc->ham_ncand, (unsigned long long)fl_n);
            }
        }
        const unsigned char *As = abase + (size_t)(ARES ? ch : buf) * F4_OP, *Bs = bbase + (size_t)buf * F4_OP;
        // (one k step at a time: unrolled, the compiler hoists all sixteen 16-byte reads of the chunk in front of the first MFMA and the
        // kernel no longer fits the 128 registers a 1024-thread workgroup has per lane; four waves per SIMD cover a step's read latency)
#pragma unroll 1
        for (int ks = 0; ks < F4_KC; ++ks) {
            fp4x8_t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint4 x = *reinterpret_cast<const uint4 *>(As + i * 32 * F4_ROW + ks * 32);
                a[i] = (fp4x8_t){(int)x.x, (int)x.y, (int)x.z, (int)x.w, 0, 0, 0, 0};
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint4 x = *reinterpret_cast<const uint4 *>(Bs + j * 32 * F4_ROW + ks * 32);
                b[j] = (fp4x8_t){(int)x.x, (int)x.y, (int)x.z, (int)x.w, 0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i], b[j], acc[i][j], 4, 4, 0, one, 0, one);
        }
        F4_STAMP(it, 1);
        if (more) {  // (the other buffers: their readers passed the barrier of the chunk before)
            if constexpr (!ARES) F4_STORE_A(buf ^ 1);
            F4_STORE_B(buf ^ 1);
        }
        F4_STAMP(it, 2);
        if (wv == 0 && fl_n != 0u) {  // (its readers here, the list's next writers behind this chunk's barrier)
            F4_STAMP(it, 6);
            F4_FLUSH_WRITE((J - 1 - J0) & 1, J - 1, fl_n, fl_base);
            fl_n = 0u;
            F4_STAMP(it, 7);
        }
        if (last) {
            F4_STAMP(it, 3);
            // ---- tile J is complete: its candidates go to its LDS list, then the accumulators start over.  No barrier and no device-wide
            // atomic here: the chunk's barrier below publishes the list, wave 0 flushes it under the next chunk ----
            // accumulator element e of block (i, j): row 8 (e / 4) + 4 (lane / 32) + e % 4, column lane % 32
            const int slot_n = (J - J0) & 1;
            const bool diag = I == J;
            unsigned long long cand[2] = {0ull, 0ull};  // bit 16 j + e of cand[i]: element e of block (i, j)
            // One compare per accumulator, its lane mask tested on the scalar side: a tile lists a few dozen of its 65 536 pairs, so
            // nearly every mask is empty and the validity tests run for the few that are not.  (As one maximum per lane and then the
            // whole scan wherever any lane of the wave held a candidate -- nearly every wave of every tile at C -- the scan's vector
            // instructions were half of a tile's time: profiles/fp4_feed_stamps_C.txt.)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e4 = 0; e4 < 16; e4 += 4) {
                        // (four accumulators share the first test: a compare and a branch each cost a wave about 12 clocks)
                        const float m4 = fmaxf(fmaxf(acc[i][j][e4], acc[i][j][e4 + 1]), fmaxf(acc[i][j][e4 + 2], acc[i][j][e4 + 3]));
                        if (__builtin_amdgcn_ballot_w64(m4 > limit) != 0ull) {  // (wave-uniform)
#pragma unroll
                            for (int e = e4; e < e4 + 4; ++e) {
                                const bool above = acc[i][j][e] > limit;
                                if (__builtin_amdgcn_ballot_w64(above) != 0ull) {  // (wave-uniform)
                                    // (the empty asm: without it the compiler keeps all 64 row indices in registers for the whole walk)
                                    int rb = I * F4_TILE + wr * 64 + 4 * lh;
                                    asm volatile("" : "+v"(rb));
                                    const int gr = rb + i * 32 + 8 * (e >> 2) + (e & 3);
                                    const int gc = J * F4_TILE + wc * 64 + j * 32 + l32;
                                    if (above && gr < M && gc < M && (diag ? gr < gc : true)) cand[i] |= 1ull << (16 * j + e);
                                }
                            }
                        }
#pragma unroll
                        for (int e = e4; e < e4 + 4; ++e) acc[i][j][e] = 0.f;
                    }
            F4_STAMP(it, 8);
            const unsigned mine = (unsigned)(__builtin_popcountll(cand[0]) + __builtin_popcountll(cand[1]));
            if (__builtin_amdgcn_ballot_w64(mine != 0u) != 0ull) {  // (wave-uniform)
                // the wave's candidates take one run of the list: a prefix sum over its lanes, one LDS atomic
                unsigned incl = mine;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned v = __shfl_up(incl, d);
                    if (lane >= d) incl += v;
                }
                const unsigned wtot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
                unsigned woff = 0u;
                if (lane == 0) woff = atomicAdd(&f4_cnt[slot_n], wtot);
                woff = (unsigned)__builtin_amdgcn_readfirstlane((int)woff);
                // what of the run lies beyond the LDS list (a tile of a cluster may hold up to 65 536 candidates) goes straight to the
                // global list, with an atomic of this wave's own
                const unsigned spill0 = max(woff, (unsigned)F4_LCAP);
                const unsigned nspill = woff + wtot > spill0 ? woff + wtot - spill0 : 0u;
                unsigned gbase = 0u;
                if (nspill != 0u) {
                    unsigned long long b64 = 0ull;
                    if (lane == 0) b64 = atomicAdd(&sc->ham_ncand, (unsigned long long)nspill);
                    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b64 & 0xffffffffull));
                    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b64 >> 32));
                    gbase = (hi != 0u || lo > cand_cap) ? cand_cap : lo;  // (beyond the capacity nothing is written)
                }
                F4_STAMP(it, 9);
                unsigned idx = woff + incl - mine;
                unsigned *lst = f4_list + slot_n * F4_LCAP;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    unsigned long long c = cand[i];
                    while (c) {
                        const int bit = __builtin_ctzll(c), j = bit >> 4, e = bit & 15;
                        const int tr = wr * 64 + i * 32 + 8 * (e >> 2) + 4 * lh + (e & 3), tc = wc * 64 + j * 32 + l32;
                        if (idx < (unsigned)F4_LCAP) {
                            lst[idx] = (unsigned)(tr << 8 | tc);
                        } else {
                            const unsigned slot = gbase + (idx - spill0);
                            if (slot < cand_cap) cand_list[slot] = make_int2(I * F4_TILE + tr, J * F4_TILE + tc);
                        }
                        ++idx;
                        c &= c - 1;
                    }
                }
            }
            F4_STAMP(it, 4);
        }
        J = Jn;
        ch = chn;
        __syncthreads();
        F4_STAMP(it, 5);
    }
    // the walk's last tile: published by the loop's last barrier
    if (wv == 0) {
        const int q = (J1 - 1 - J0) & 1;
        const unsigned n = min(f4_cnt[q], (unsigned)F4_LCAP);
        if (n != 0u) {
            unsigned long long b64 = 0ull;
            if (lane == 0) b64 = atomicAdd(&sc->ham_ncand, (unsigned long long)n);
            F4_FLUSH_WRITE(q, J1 - 1, n, b64);
        }
    }
#undef F4_FLUSH_WRITE
}

// ---- how many pairs would this form list?  (a sample of 128 x 128 tiles, the very tiles k_hamming<3, PROBE> takes for the three-plane form) ------
// D1 counted with plain popcounts of the image's sign bits: 192 tiles, microseconds.  sc->ham_cand2 += pairs of the sampled tiles with
// D1 < thresh (a diagonal tile's pairs twice, as the three-plane probe counts them).
#define F4_PW 8  // words per round of the probe
struct k_fp4_probe_args {
    const uint4 *img;
    int E, NW, M, Mt;  // Mt: 128-tiles per side
    gdca_dev_scalars *sc;
};
template <int CAP>
__global__ __launch_bounds__(256) void k_fp4_probe(const BatchArgs<k_fp4_probe_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const uint4 *__restrict__ img = a_.img;
    const int E = a_.E, NW = a_.NW, M = a_.M, Mt = a_.Mt;
    gdca_dev_scalars *sc = a_.sc;
    const int thresh = sc->thresh;
    if (thresh <= 0) return;
    __shared__ int total;
    __shared__ uint32_t bits[2][F4_PW][128];  // [operand][word of the round][row of the tile]
    int I, J;
    // (gridDim.x tiles spread evenly over the upper triangle's Mt (Mt + 1) / 2)
    f4_tri_decode((int)(((long long)blockIdx.x * ((long long)Mt * (Mt + 1) / 2)) / gridDim.x), Mt, I, J);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid == 0) total = 0;
    int D[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) D[r][c] = 0;
    // thread t < 128: row t of tile row I; else row t - 128 of tile row J (the image's rows are padded to 256: in bounds)
    const uint4 *mine = img + (size_t)((tid < 128 ? I : J) * 128 + (tid & 127)) * E;
    for (int w0 = 0; w0 < NW; w0 += F4_PW) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < F4_PW; ++u) {
            uint32_t b = 0u;
            if (w0 + u < NW) {
                const uint4 v = mine[w0 + u];
                b = f4_signs8(v.x) | (f4_signs8(v.y) << 8) | (f4_signs8(v.z) << 16) | (f4_signs8(v.w) << 24);
            }
            bits[tid >> 7][u][tid & 127] = b;
        }
        __syncthreads();
        const int wn = min(F4_PW, NW - w0);
        for (int u = 0; u < wn; ++u) {
            uint32_t a[8], b[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) a[r] = bits[0][u][ty * 8 + r];
#pragma unroll
            for (int c = 0; c < 8; ++c) b[c] = bits[1][u][tx * 8 + c];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) D[r][c] += __builtin_popcount(a[r] ^ b[c]);
        }
    }
    int cand = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int gr = I * 128 + ty * 8 + r, gc = J * 128 + tx * 8 + c;
            cand += (gr < M) && (gc < M) && (gr != gc) && (D[r][c] < thresh);
        }
    if (cand) atomicAdd(&total, cand);
    __syncthreads();
    if (tid == 0 && total) atomicAdd(&sc->ham_cand2, total);
}

// sigma and the image: before the probe and the decision (the probe reads the image), for every family that may take this form
void gdca_launch_hamming_fp4_image(hipStream_t s, const int8_t *Z, const uint32_t *hist, void *img, int N, int M)
{
    const int NW = (N + 31) / 32, E = f4_entries(NW), rows = (M + F4_TILE - 1) / F4_TILE * F4_TILE;
    uint8_t *sigma = (uint8_t *)img + f4_image_only_bytes(N, M);
    gdca_launch<k_fp4_sigma_args, k_fp4_sigma<1>, k_fp4_sigma<GDCA_MAXB>>(dim3((unsigned)((32 * E + 255) / 256)), dim3(256), 0, s, k_fp4_sigma_args{hist, sigma, N, 32 * E});
    const long long items = (long long)rows * E;
    gdca_launch<k_fp4_image_args, k_fp4_image<1>, k_fp4_image<GDCA_MAXB>>(dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s,
                                                                           k_fp4_image_args{Z, sigma, (uint4 *)img, N, M, E, rows});
}

void gdca_launch_hamming_fp4_probe(hipStream_t s, const void *img, int N, int M, int nprobe, gdca_dev_scalars *sc)
{
    const int NW = (N + 31) / 32, Mt = (M + 127) / 128;
    gdca_launch<k_fp4_probe_args, k_fp4_probe<1>, k_fp4_probe<GDCA_MAXB>>(dim3((unsigned)nprobe), dim3(256), 0, s,
                                                                           k_fp4_probe_args{(const uint4 *)img, f4_entries(NW), NW, M, Mt, sc});
}

// Enqueues the tile products; they leave at once unless k_hamming_decide chose this form (sc->ham_mode == 2).
// img: the image gdca_launch_hamming_fp4_image built; cand_list / cap: the list k_hamming_refine consumes.
void gdca_launch_hamming_fp4(hipStream_t s, const void *img, int N, int M, gdca_dev_scalars *sc, void *cand_list, unsigned cap)
{
    const int NW = (N + 31) / 32, E = f4_entries(NW), Mt = (M + F4_TILE - 1) / F4_TILE;
    const dim3 grid((unsigned)((Mt + F4_SEG - 1) / F4_SEG), (unsigned)Mt);
    const k_hamming_fp4_args a{(const unsigned char *)img, E, M, Mt, N, sc, (int2 *)cand_list, cap};
    if (E <= 4 * F4_KC)
        gdca_launch<k_hamming_fp4_args, k_hamming_fp4<1, true>, k_hamming_fp4<GDCA_MAXB, true>>(grid, dim3(1024), F4_LDS_ALL, s, a);
    else
        gdca_launch<k_hamming_fp4_args, k_hamming_fp4<1, false>, k_hamming_fp4<GDCA_MAXB, false>>(grid, dim3(1024), F4_LDS_ALL, s, a);
}
