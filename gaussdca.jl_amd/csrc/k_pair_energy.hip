// All-pairs partner energies across a split alignment: the energy of every concatenation a (+) b of K_A sequences of protein A (sites
// 0 .. split - 1) with K_B sequences of protein B (the rest) under the fitted Gaussian model -- what the paper's partner matching
// ranks candidate pairings by.  With E(x) = 1/2 (x - Pi)' mJ (x - Pi) of k_energy.hip, one-hot x = xA (+) xB, g = mJ Pi, c0 = Pi' g:
//
//     E(a (+) b) = E(a (+) gaps) + E(gaps (+) b) - c0 / 2 + R(a, b)
//     R(a, b)    = sum_{i in A, j in B, neither a gap} mJ[r(j), r(i)],      r(i) = i s + a_i - 1
//
// (a gap leaves its site's block of x zero, so E(a (+) gaps) holds a's quadratic and linear terms and c0 / 2, E(gaps (+) b) holds b's
// and c0 / 2 once more, and only the cross terms -- each pair (i, j) once, from the lower triangle -- depend on the pairing).  The
// first two terms are K_A + K_B runs of the existing energy stage; R is the work of this file.  It reads ONE rectangular block of mJ:
// rows n_A .. n - 1, columns 0 .. n_A - 1, n_A = split s, wholly inside the strictly lower triangle the sweep leaves valid (there with
// the sign flipped: `sign` = -1, ld = n_pad; the operator form: sign +1, ld = n).  Nothing else of mJ is read here.
//
// Materialising the K_A K_B concatenations costs N^2 / 2 gathers a pair; here a pair costs N_B:
//   k_energy_pack  (k_energy.hip) the symbols of each half's range of sites, dwords [ceil(Ns / 4)][K], with the symbol check;
//   k_pair_pad     a (+) gaps and gaps (+) b as N x (K_A + K_B) sequences for the energy stage;
//   k_pair_fold    T[a][row] = sum_{i in A} sign A[n_A + row, r_a(i)] over the n_B rows of the block: a workgroup owns 64 rows and
//                  4 x AU sequences; it walks the A site blocks (4 sites), tile -> LDS as 4 (s + 1) columns of 64 rows (42 KB at
//                  s = 20, 62 KB at s = 30; a column segment of the block is contiguous), then each wave adds, for each of its AU
//                  sequences, the four columns the sequence's symbols select (lane = row: conflict-free, the column is wave-uniform);
//   k_pair_gather  R[a, b] = sum_{j in B} T[a][r_b(j)]: a workgroup keeps segments of the T rows of 8 sequences a in LDS, interleaved
//                  [row][8] (64 B a row: one symbol decode serves eight pairings), for 256 x BU sequences b; and, `what` = energy, the
//                  combination ((EA[a] + EB[b]) - c0 / 2) + R in its epilogue -- the K_A x K_B matrix is written once and never read.
//                  A third compile-time variant (LO) carries the energy on to the LOG-ODDS of the pairing against the two marginal
//                  models (include/gdca.h, pair log-odds): e formed exactly as above, then ((EmA[a] + EmB[b]) - e) + I, with the
//                  marginal energies read like EA / EB and I a kernel argument from the host; e is never stored.
//   k_pair_gather_blocked  the same sum for the pairings INSIDE the species of a species-sorted problem (include/gdca.h, partner
//                  matching): a work item = (species, up to 8 of its sequences a, up to 32 of its sequences b), built on the host;
//                  the same LDS layout, segments and epilogue, but a lane owns ONE pairing (lane = (b, a of 8)) where k_pair_gather's
//                  lane owns a sequence b against eight a -- a species of five would use five of its lanes.  The packed block of
//                  species s is written once.  Every entry is bit for bit k_pair_gather's (the same additions in the same order).
// T is chunked over a (gdca_pair_chunk: ~256 MB; option PAIR_CHUNK).
// ORDER-FIXED: T[a][row] is summed by ONE thread over the sites i ascending, R[a, b] by ONE thread over the sites j ascending (the
// segments in ascending order), gaps adding an exact zero in their place; the fold direction is always A.  No floating-point atomics.
// So E[a, b] is the same bits from run to run, whatever K_A and K_B are, wherever a and b stand in their batches, however T is
// chunked and whichever instance (AU, BU) runs.  (The only atomic is the integer OR of the bad-symbol flag.)
#include "gdca_internal.h"
#include "gdca_launch.h"

#define PT 4          // sites per tile of k_pair_fold (= symbols per packed dword: k_energy_pack's four)
#define PROWS 64      // rows of the block per workgroup of k_pair_fold
#define PAU_WIDE 32   // sequences a per wave of k_pair_fold ...
#define PAU_NARROW 4  // ... and where that would leave compute units without a workgroup
#define PGA 8         // sequences a whose T rows a workgroup of k_pair_gather holds
#define PBU_WIDE 2    // sequences b per thread of k_pair_gather / where that would leave compute units without a workgroup
#define PBU_NARROW 1
#define PGB 32        // sequences b of one work item of k_pair_gather_blocked (x PGA sequences a: the workgroup's 256 lanes)
#define PSEG_ROWS 1020  // T rows per LDS segment of k_pair_gather: (1020 + 1) x 8 doubles = 63.8 KB, two workgroups a compute unit

// Xp (N x (KA + KB)): sequence k < KA = a_k (+) gaps, sequence KA + k = gaps (+) b_k (bytes copied as they are: the energy stage's own
// pack flags an illegal one)
__global__ __launch_bounds__(256) void k_pair_pad(const int8_t *__restrict__ XA, size_t strideA, const int8_t *__restrict__ XB,
                                                  size_t strideB, int N, int split, int KA, int KB, int q, int8_t *__restrict__ Xp)
{
    // (a grid-stride loop: N (KA + KB) bytes can be more than one grid's threads)
    const size_t total = (size_t)N * ((size_t)KA + (size_t)KB), step = (size_t)gridDim.x * 256;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += step) {
        const size_t k = idx / (size_t)N;
        const int i = (int)(idx - k * (size_t)N);
        int8_t v = (int8_t)q;
        if (k < (size_t)KA) {
            if (i < split) v = XA[k * strideA + i];
        } else if (i >= split) {
            v = XB[(k - (size_t)KA) * strideB + (i - split)];
        }
        Xp[idx] = v;
    }
}

// ---- fold A ------------------------------------------------------------------------------------------------------------------------------
struct k_pair_fold_args {
    const double *A;  // element (row, col) at A[col * ld + row]; the block: rows nA .. nA + nB - 1, columns 0 .. nA - 1
    size_t ld;
    double sign;
    const uint32_t *XAg;  // [ceil(NA / 4)][KA]
    double *T;            // [Ac][nB]: this launch's sequences a0 .. a0 + Ac - 1
    int NA, sdim, nA, nB, KA, a0, Ac;
};

// AU: sequences per wave.  It does not change the order of any sum.
template <int AU>
__global__ __launch_bounds__(256) void k_pair_fold(const k_pair_fold_args p)
{
    extern __shared__ double lds_[];  // [TD columns][64 rows]
    const int sdim = p.sdim, s1 = sdim + 1, TD = PT * s1;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int row = (int)blockIdx.x * PROWS + lane;
    const bool rok = row < p.nB;
    const double *__restrict__ Ar = p.A + (size_t)p.nA + (size_t)(rok ? row : 0);
    const size_t ld = p.ld;
    const int ab = (int)blockIdx.y * (4 * AU) + wave * AU;  // this wave's first sequence, within the launch's Ac
    const uint32_t gapw = 0x01010101u * (uint32_t)sdim;
    double acc[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) acc[u] = 0.0;

    const int nJ = (p.NA + PT - 1) / PT;
    for (int J = 0; J < nJ; ++J) {
        __syncthreads();  // (the previous tile has been read)
        for (int c0 = wave; c0 < TD; c0 += 16) {
            double v[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int c = c0 + 4 * b;
                const int jl = c / s1, ca = c - jl * s1, site = J * PT + jl;
                const bool ok = rok && c < TD && ca < sdim && site < p.NA;
                v[b] = ok ? p.sign * Ar[(size_t)(site * sdim + ca) * ld] : 0.0;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int c = c0 + 4 * b;
                if (c < TD) lds_[c * PROWS + lane] = v[b];
            }
        }
        // the symbols of this wave's sequences at the tile's four sites: lane u holds sequence u's
        uint32_t w = gapw;
        if (lane < AU && ab + lane < p.Ac) w = p.XAg[(size_t)J * p.KA + p.a0 + ab + lane];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const uint32_t wu = (uint32_t)__builtin_amdgcn_readlane((int)w, u);
#pragma unroll
            for (int l = 0; l < PT; ++l) acc[u] += lds_[(l * s1 + (int)((wu >> (8 * l)) & 0xffu)) * PROWS + lane];
        }
    }
    if (rok) {
#pragma unroll
        for (int u = 0; u < AU; ++u)
            if (ab + u < p.Ac) p.T[(size_t)(ab + u) * p.nB + row] = acc[u];
    }
}

// ---- gather B, and the combination -----------------------------------------------------------------------------------------------------
struct k_pair_gather_args {
    const double *T;      // [Ac][nB]
    const uint32_t *XBg;  // [ceil(NB / 4)][KB]
    const double *EAB;    // what = energy: E(a (+) gaps) [KA], then E(gaps (+) b) [KB]; else nullptr
    const double *c0;
    double *E;            // [KB][KA]: E[a + KA * b]
    int NB, sdim, nB, SB, KA, KB, a0, Ac, b0;
    gdca_logodds_terms lo;  // the LO instances: the marginal models' energies EmA [KA], EmB [KB] and the constant I
};

template <int BU, bool LO>
__global__ __launch_bounds__(256) void k_pair_gather(const k_pair_gather_args p)
{
    extern __shared__ double lds_[];  // [SR + 1 rows][PGA]: a segment of the T rows of this workgroup's sequences a; row SR = zeros (the gap)
    const int sdim = p.sdim, SR = p.SB * sdim;
    const int t = threadIdx.x;
    const int ag = (int)blockIdx.x * PGA;  // first sequence a, within the launch's Ac
    long long bk[BU];
    double acc[BU][PGA];
#pragma unroll
    for (int u = 0; u < BU; ++u) {
        bk[u] = (long long)p.b0 + (long long)blockIdx.y * (256 * BU) + 256 * u + t;
#pragma unroll
        for (int g = 0; g < PGA; ++g) acc[u][g] = 0.0;
    }
    const uint32_t gapw = 0x01010101u * (uint32_t)sdim;

    for (int j0 = 0; j0 < p.NB; j0 += p.SB) {
        const int r0 = j0 * sdim;
        const int nr = min(SR, p.nB - r0);
        __syncthreads();  // (the previous segment has been read)
        for (int idx = t; idx < nr * PGA; idx += 256) {
            const int g = idx & (PGA - 1), r = idx >> 3;
            lds_[idx] = ag + g < p.Ac ? p.T[(size_t)(ag + g) * p.nB + r0 + r] : 0.0;
        }
        if (t < PGA) lds_[SR * PGA + t] = 0.0;
        __syncthreads();
        const int nw = (min(p.SB, p.NB - j0) + PT - 1) / PT;
        for (int jb = 0; jb < nw; ++jb) {
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const uint32_t w = bk[u] < p.KB ? p.XBg[(size_t)(j0 / PT + jb) * p.KB + bk[u]] : gapw;
#pragma unroll
                for (int l = 0; l < PT; ++l) {
                    const int sym = (int)((w >> (8 * l)) & 0xffu);
                    const int r = sym < sdim ? (jb * PT + l) * sdim + sym : SR;
                    const double *src = lds_ + r * PGA;
#pragma unroll
                    for (int g = 0; g < PGA; ++g) acc[u][g] += src[g];
                }
            }
        }
    }
    const double hc0 = p.EAB ? 0.5 * *p.c0 : 0.0;
#pragma unroll
    for (int u = 0; u < BU; ++u) {
        if (bk[u] >= p.KB) continue;
        const double eb = p.EAB ? p.EAB[(size_t)p.KA + bk[u]] : 0.0;
        double emb = 0.0;
        if constexpr (LO) emb = p.lo.EmB[bk[u]];
#pragma unroll
        for (int g = 0; g < PGA; ++g) {
            if (ag + g >= p.Ac) continue;
            const int a = p.a0 + ag + g;
            const double r = acc[u][g];
            const double e = p.EAB ? ((p.EAB[a] + eb) - hc0) + r : r;
            if constexpr (LO)
                p.E[(size_t)a + (size_t)p.KA * (size_t)bk[u]] = ((p.lo.EmA[a] + emb) - e) + p.lo.I;
            else
                p.E[(size_t)a + (size_t)p.KA * (size_t)bk[u]] = e;
        }
    }
}

// ---- gather B inside the species of a species-sorted problem ------------------------------------------------------------------------------
struct k_pair_gather_blocked_args {
    const double *T;      // [Ac][nB]
    const uint32_t *XBg;  // [ceil(NB / 4)][KB]
    const double *EAB;    // as k_pair_gather
    const double *c0;
    double *E;            // packed: block s at eoff[s], column-major kA_s x kB_s
    const int4 *items;    // this launch's work items: x = species, y = first a (global), z = first b (global), w = na | nb << 8
    const long long *eoff;  // [S + 1]
    const int *offA, *offB;  // [S + 1] each
    int NB, sdim, nB, SB, KA, KB, a0;
    gdca_logodds_terms lo;  // as k_pair_gather
};

template <bool LO>
__global__ __launch_bounds__(256) void k_pair_gather_blocked(const k_pair_gather_blocked_args p)
{
    extern __shared__ double lds_[];  // as k_pair_gather: [SR + 1 rows][PGA], row SR = zeros (the gap)
    const int sdim = p.sdim, SR = p.SB * sdim;
    const int t = threadIdx.x, g = t & (PGA - 1), bl = t >> 3;
    const int4 it = p.items[blockIdx.x];
    const int na = it.w & 0xff, nb = it.w >> 8;
    const int ag = it.y - p.a0;  // first sequence a, within the launch's Ac (the host cuts the groups at the chunk boundaries)
    const bool live = g < na && bl < nb;
    const long long bk = (long long)it.z + bl;
    double acc = 0.0;
    const uint32_t gapw = 0x01010101u * (uint32_t)sdim;

    for (int j0 = 0; j0 < p.NB; j0 += p.SB) {
        const int r0 = j0 * sdim;
        const int nr = min(SR, p.nB - r0);
        __syncthreads();  // (the previous segment has been read)
        for (int idx = t; idx < nr * PGA; idx += 256) {
            const int gg = idx & (PGA - 1), r = idx >> 3;
            lds_[idx] = gg < na ? p.T[(size_t)(ag + gg) * p.nB + r0 + r] : 0.0;
        }
        if (t < PGA) lds_[SR * PGA + t] = 0.0;
        __syncthreads();
        const int nw = (min(p.SB, p.NB - j0) + PT - 1) / PT;
        for (int jb = 0; jb < nw; ++jb) {
            const uint32_t w = live ? p.XBg[(size_t)(j0 / PT + jb) * p.KB + bk] : gapw;
#pragma unroll
            for (int l = 0; l < PT; ++l) {
                const int sym = (int)((w >> (8 * l)) & 0xffu);
                const int r = sym < sdim ? (jb * PT + l) * sdim + sym : SR;
                acc += lds_[r * PGA + g];
            }
        }
    }
    if (!live) return;
    const int a = it.y + g, oa = p.offA[it.x];
    const long long kA = p.offA[it.x + 1] - oa;
    const size_t at = (size_t)(p.eoff[it.x] + (a - oa) + kA * (bk - p.offB[it.x]));
    if (p.EAB) {
        const double hc0 = 0.5 * *p.c0;
        const double e = ((p.EAB[a] + p.EAB[(size_t)p.KA + bk]) - hc0) + acc;
        if constexpr (LO)
            p.E[at] = ((p.lo.EmA[a] + p.lo.EmB[bk]) - e) + p.lo.I;
        else
            p.E[at] = e;
    } else {
        p.E[at] = acc;
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
// sequences a one launch of the fold / gather kernels takes: a multiple of the fold workgroup's 4 x PAU_WIDE whose T stays within
// ~256 MB, at most 32768 (wanted > 0: option PAIR_CHUNK, any SMALLER count -- tests; it never raises the buffer beyond the rule)
int gdca_pair_chunk(int nB, int KA, int wanted)
{
    const long long per = 4 * PAU_WIDE, cap = 32768;
    long long kc = ((long long)256 << 20) / ((long long)nB * 8) / per * per;
    if (kc < per) kc = per;
    if (kc > cap) kc = cap;
    if (wanted > 0 && wanted < kc) kc = wanted;
    return (int)(kc < KA ? kc : KA);
}

void gdca_launch_pair_pad(hipStream_t s, const int8_t *XA, size_t strideA, const int8_t *XB, size_t strideB, int N, int split, int KA, int KB,
                          int q, int8_t *Xp)
{
    const size_t total = (size_t)N * ((size_t)KA + (size_t)KB);
    const size_t blocks = (total + 255) / 256;
    GDCA_LAUNCH_DIRECT(k_pair_pad, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, s, XA, strideA, XB, strideB, N, split, KA, KB, q, Xp);
}

// T[a0 .. a0 + Ac - 1][nB rows] from the block of A (ld, sign) and the packed symbols of the A halves
static hipError_t launch_pair_fold(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *XAg, int NA, int NB, int sdim, int KA,
                                   int a0, int Ac, double *T, int ncu)
{
    const int nA = NA * sdim, nB = NB * sdim;
    const k_pair_fold_args a{A, ld, sign, XAg, T, NA, sdim, nA, nB, KA, a0, Ac};
    const int rt = (nB + PROWS - 1) / PROWS;
    // 128 sequences a workgroup -- or 16, where 128 would give fewer than two workgroups a compute unit
    const bool wide = gdca_wide_instance(Ac, 4 * PAU_WIDE, rt, ncu);
    const int per = 4 * (wide ? PAU_WIDE : PAU_NARROW);
    const size_t lds = (size_t)PT * (sdim + 1) * PROWS * sizeof(double);
    void (*kern)(k_pair_fold_args) = wide ? k_pair_fold<PAU_WIDE> : k_pair_fold<PAU_NARROW>;
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, dim3(rt, (Ac + per - 1) / per), dim3(256), lds, s, a);
    return hipSuccess;
}

// sites per LDS segment of the gather kernels: whole dwords of XBg (s <= 30: at least 32)
static int pair_segment_sites(int NB, int sdim)
{
    int SB = (PSEG_ROWS / sdim) & ~(PT - 1);
    if (SB > ((NB + PT - 1) & ~(PT - 1))) SB = (NB + PT - 1) & ~(PT - 1);
    return SB;
}

// E[a0 .. a0 + Ac - 1][all b] from the block of A (ld, sign) and the packed symbols; T: Ac x nB doubles.  EAB == nullptr: the coupling R.
// An error: the dynamic LDS limit could not be raised for a tile; the kernel it was for and those behind it were not launched
hipError_t gdca_launch_pair_chunk(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *XAg, const uint32_t *XBg, int N, int split,
                            int sdim, int KA, int KB, int a0, int Ac, double *T, const double *EAB, const double *c0, double *E, int ncu,
                            const gdca_logodds_terms *lo)
{
    const int NB = N - split, nB = NB * sdim;
    {
        const hipError_t e = launch_pair_fold(s, A, ld, sign, XAg, split, NB, sdim, KA, a0, Ac, T, ncu);
        if (e != hipSuccess) return e;
    }
    {
        const int SB = pair_segment_sites(NB, sdim);
        const size_t lds = ((size_t)SB * sdim + 1) * PGA * sizeof(double);
        const int ga = (Ac + PGA - 1) / PGA;
        const bool wide = gdca_wide_instance(KB, 256 * PBU_WIDE, ga, ncu);
        const int per = 256 * (wide ? PBU_WIDE : PBU_NARROW);
        void (*kern)(k_pair_gather_args) = lo ? (wide ? k_pair_gather<PBU_WIDE, true> : k_pair_gather<PBU_NARROW, true>)
                                              : (wide ? k_pair_gather<PBU_WIDE, false> : k_pair_gather<PBU_NARROW, false>);
        const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        const long long maxb = (long long)65535 * per;  // sequences b one launch's grid covers
        for (long long b0 = 0; b0 < KB; b0 += maxb) {
            const long long kb = KB - b0 < maxb ? KB - b0 : maxb;
            const k_pair_gather_args a{T, XBg, EAB, c0, E, NB, sdim, nB, SB, KA, KB, a0, Ac, (int)b0, lo ? *lo : gdca_logodds_terms{}};
            GDCA_LAUNCH_DIRECT(kern, dim3(ga, (unsigned)((kb + per - 1) / per)), dim3(256), lds, s, a);
        }
    }
    return hipSuccess;
}

// The work list of the blocked gather for species-sorted sequences (offA / offB: S + 1 valid offsets): items (species, first a, first b,
// na | nb << 8) of up to PGA sequences a and PGB sequences b of one species, a ascending; a group of a never crosses a multiple of
// `Ac` (the chunks of T).  first[c] = the first item of chunk c, c = 0 .. ceil(KA / Ac) (the last entry: all).  Empty sides give none.
void gdca_pair_block_items(const int32_t *offA, const int32_t *offB, int S, int Ac, std::vector<int32_t> &items, std::vector<long long> &first)
{
    items.clear();
    first.assign(1, 0);
    const int KA = offA[S];
    int s = 0;
    for (int c0 = 0; c0 < KA; c0 += Ac) {
        const int c1 = KA - c0 < Ac ? KA : c0 + Ac;
        while (s < S && offA[s + 1] <= c0) ++s;
        for (int sp = s; sp < S && offA[sp] < c1; ++sp) {
            const int lo = offA[sp] > c0 ? offA[sp] : c0, hi = offA[sp + 1] < c1 ? offA[sp + 1] : c1;
            if (offB[sp + 1] == offB[sp]) continue;
            for (int a = lo; a < hi; a += PGA)
                for (int b = offB[sp]; b < offB[sp + 1]; b += PGB) {
                    const int na = hi - a < PGA ? hi - a : PGA, nb = offB[sp + 1] - b < PGB ? offB[sp + 1] - b : PGB;
                    const int32_t it[4] = {sp, a, b, na | nb << 8};
                    items.insert(items.end(), it, it + 4);
                }
        }
        first.push_back((long long)(items.size() / 4));
    }
}

// The blocks of E of the species whose sequences a lie in a0 .. a0 + Ac - 1, from `nitems` work items of that chunk (device; eoff,
// offA, offB: the species table on the device).  The fold is gdca_launch_pair_chunk's own.
hipError_t gdca_launch_pair_chunk_blocked(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *XAg, const uint32_t *XBg, int N,
                                          int split, int sdim, int KA, int KB, int a0, int Ac, double *T, const double *EAB, const double *c0,
                                          double *E, const int32_t *items, long long nitems, const long long *eoff, const int32_t *offA,
                                          const int32_t *offB, int ncu, const gdca_logodds_terms *lo)
{
    const int NB = N - split, nB = NB * sdim;
    if (nitems == 0) return hipSuccess;  // (no pairing of these sequences a is wanted: their rows need not be folded)
    const hipError_t e = launch_pair_fold(s, A, ld, sign, XAg, split, NB, sdim, KA, a0, Ac, T, ncu);
    if (e != hipSuccess) return e;
    const int SB = pair_segment_sites(NB, sdim);
    const size_t lds = ((size_t)SB * sdim + 1) * PGA * sizeof(double);
    void (*kern)(k_pair_gather_blocked_args) = lo ? k_pair_gather_blocked<true> : k_pair_gather_blocked<false>;
    const hipError_t e2 = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e2 != hipSuccess) return e2;
    const long long maxi = 1 << 30;  // items one launch's grid covers
    for (long long i0 = 0; i0 < nitems; i0 += maxi) {
        const long long ni = nitems - i0 < maxi ? nitems - i0 : maxi;
        const k_pair_gather_blocked_args a{T, XBg, EAB, c0, E, reinterpret_cast<const int4 *>(items) + i0, eoff, offA, offB, NB, sdim, nB, SB, KA, KB, a0,
                                           lo ? *lo : gdca_logodds_terms{}};
        GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)ni), dim3(256), lds, s, a);
    }
    return hipSuccess;
}

// ---- the negation for the assignment on log-odds -------------------------------------------------------------------------------------------
// dst[i] = -src[i] over the packed blocks: the assignment MAXIMISES the total log-odds of a species by minimising -L (exact)
__global__ __launch_bounds__(256) void k_negate(const double *__restrict__ src, double *__restrict__ dst, size_t len)
{
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < len; i += step) dst[i] = -src[i];
}

void gdca_launch_negate(hipStream_t s, const double *src, double *dst, size_t len)
{
    if (len == 0) return;
    const size_t blocks = (len + 255) / 256;
    GDCA_LAUNCH_DIRECT(k_negate, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, s, src, dst, len);
}
