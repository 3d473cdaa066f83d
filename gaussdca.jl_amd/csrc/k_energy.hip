// Energies of sequences under the fitted Gaussian model: the other use of mJ = inv(cholesky(C)) (src/GaussDCA.jl:34) -- the
// paper's "protein-interaction partners" half scores sequences by their likelihood under the multivariate Gaussian whose
// covariance src/GaussDCA.jl:32 builds.  With the project's one-hot encoding x (x[i*s + a - 1] = 1 for symbol a in 1..s at site i,
// the gap q leaves the site's block zero) and Pi the single-site frequencies with pseudocount (:30):
//
//     E(x) = 1/2 (x - Pi)' mJ (x - Pi)
//          = 1/2 ( sum_i sum_j mJ[r(i), r(j)]  -  2 sum_i g[r(i)]  +  c0 ),   g = mJ Pi,  c0 = Pi' g,  r(i) = i s + a_i - 1
//
// (sums over the non-gap sites).  This is minus the log-likelihood up to the model's constant 1/2 log det(2 pi C), which is OUT OF
// SCOPE here: the block sweep does not produce the Cholesky pivots, and comparisons inside one model never need it.  Lower = fits better.
//
// mJ is symmetric and only its element-wise lower triangle is read (what the sweep leaves valid in ctx->A, there with the sign
// flipped: `sign` = -1):  E = sum_{i>j} mJ[r(i), r(j)] + sum_i (mJ[r(i), r(i)] / 2 - g[r(i)]) + c0 / 2.
//
// Per sequence that is a gather of N^2 / 2 doubles from a matrix that fits no cache, so the gathers are turned into LDS reads:
//   k_energy_pack   X [K][N] -> Xg [ceil(N / 4)][K] dwords: the four symbols of a site block as LDS row indices a - 1 (gap, a site
//                   beyond N and an illegal byte -> s, a row of zeros); illegal bytes are flagged (sc->bad_symbol, GDCA_BAD_SEQUENCE) HERE, so
//                   nothing downstream can index out of bounds (the one pack kernel: the pair energies and the mutation scan
//                   pack with it too, the former a range of sites with a stride of its own);
//   k_energy_gtile / _gfin / _c0   g and c0 in one streaming pass over the lower triangle (64 x 64 tiles, each giving its rows' and,
//                   transposed, its columns' partial products; partials summed in tile order);
//   k_energy_rows   a workgroup owns site block I (4 sites) and 256 x SEQ sequences; it walks the tiles (I, J), J = 0 .. I, of the
//                   lower triangle: tile -> LDS as (4 (s + 1))^2 doubles (56 KB at s = 20, 123 KB at s = 30), then every thread
//                   gathers its sequences' 16 entries (one dword of Xg per sequence and tile gives the four column symbols; the row
//                   symbols stay in registers over the whole walk);
//   k_energy_final  E[k] = sum_I part[I][k] + c0 / 2.
// ORDER-FIXED: a sequence's sum is taken by ONE thread in the order J ascending, (column site, row site) ascending inside a tile,
// then over I ascending; g and c0 by fixed trees.  No floating-point atomics.  So an energy is the same bits from run to run and
// whatever else shares the batch, wherever the sequence stands in it.  (The only atomic is the integer OR of the bad-symbol flag.)
#include "gdca_internal.h"
#include "gdca_launch.h"

#define ET 4         // sites per side of a tile of k_energy_rows
#define ESEQ_WIDE 8    // sequences per thread of k_energy_rows ...
#define ESEQ_NARROW 2  // ... and where that would leave compute units without a workgroup (small N or K)
#define GT 64        // tile edge of the g pass

// ---- Ns sites of X -> packed LDS row indices, with the symbol check ---------------------------------------------------------------
// X points at the first site of the range in sequence 0; sequence k starts `stride` bytes on (whole sequences: stride = Ns = N; a
// half of a split alignment, k_pair_energy.hip: its own site count, and Z's own columns serve as they lie with stride N)
__global__ __launch_bounds__(256) void k_energy_pack(const int8_t *__restrict__ X, size_t stride, int Ns, int K, int q,
                                                     uint32_t *__restrict__ Xg, gdca_dev_scalars *sc)
{
    const int k = blockIdx.x * 256 + threadIdx.x, blk = blockIdx.y;
    if (k >= K) return;
    const int sdim = q - 1;
    uint32_t w = 0;
    bool bad = false;
#pragma unroll
    for (int l = 0; l < ET; ++l) {
        const int i = blk * ET + l;
        int idx = sdim;
        if (i < Ns) {
            const int a = X[(size_t)k * stride + i];
            if (a < 1 || a > q)
                bad = true;
            else
                idx = a - 1;
        }
        w |= (uint32_t)idx << (8 * l);
    }
    Xg[(size_t)blk * K + k] = w;
    if (bad) atomicOr(&sc->bad_symbol, GDCA_BAD_SEQUENCE);
}

// ---- g = mJ Pi from the lower triangle ----------------------------------------------------------------------------------------------
// part[o][b * 64 + x]: what block o contributes to entry x of block b -- o < b: tile (b, o) read along its rows; o > b: tile (o, b)
// read along its columns; o == b: the diagonal tile, both.  Every slot is written exactly once.
__global__ __launch_bounds__(256) void k_energy_gtile(const double *__restrict__ A, size_t ld, int n, const double *__restrict__ Pi,
                                                      double *__restrict__ part, size_t ldp)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    __shared__ double tile[GT][GT + 1];
    __shared__ double pr[GT], pc[GT];
    const int t = threadIdx.x, r = t & (GT - 1), cq = t >> 6;
    const int row = bi * GT + r;
    for (int cc = 0; cc < GT / 4; ++cc) {
        const int c = cq * (GT / 4) + cc, col = bj * GT + c;
        double v = 0.0;
        if (row < n && col < n && row >= col) v = A[(size_t)col * ld + row];
        tile[c][r] = v;
    }
    if (t < GT) pr[t] = (bi * GT + t < n) ? Pi[bi * GT + t] : 0.0;
    else if (t < 2 * GT) pc[t - GT] = (bj * GT + t - GT < n) ? Pi[bj * GT + t - GT] : 0.0;
    __syncthreads();
    double acc = 0.0;
    if (t < GT) {
        // row t of the tile (the upper part of a diagonal tile is zero)
        for (int c = 0; c < GT; ++c) acc += tile[c][t] * pc[c];
        if (bi != bj) part[(size_t)bj * ldp + (size_t)bi * GT + t] = acc;
    } else if (t < 2 * GT) {
        // column t - 64, transposed: the rows strictly below the diagonal in a diagonal tile
        const int c = t - GT;
        for (int rr = (bi == bj ? c + 1 : 0); rr < GT; ++rr) acc += tile[c][rr] * pr[rr];
        if (bi != bj) part[(size_t)bi * ldp + (size_t)bj * GT + c] = acc;
    }
    if (bi == bj) {
        // (uniform in the workgroup) a diagonal tile's two halves meet in one slot
        __syncthreads();
        if (t >= GT && t < 2 * GT) pc[t - GT] = acc;
        __syncthreads();
        if (t < GT) part[(size_t)bi * ldp + (size_t)bi * GT + t] = acc + pc[t];
    }
}

__global__ __launch_bounds__(256) void k_energy_gfin(const double *__restrict__ part, size_t ldp, int nb, int n, double sign,
                                                     double *__restrict__ g)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double acc = 0.0;
    for (int o = 0; o < nb; ++o) acc += part[(size_t)o * ldp + r];
    g[r] = sign * acc;
}

// c0 = Pi' g by one workgroup: strided partial sums, then a fixed tree
__global__ __launch_bounds__(256) void k_energy_c0(const double *__restrict__ Pi, const double *__restrict__ g, int n, double *c0)
{
    __shared__ double red[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int r = t; r < n; r += 256) acc += Pi[r] * g[r];
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) *c0 = red[0];
}

// ---- the gathers ----------------------------------------------------------------------------------------------------------------------
struct k_energy_rows_args {
    const double *A;   // mJ (sign +1) or -mJ (sign -1): element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const double *g;
    const uint32_t *Xg;  // [nI][K]
    double *part;        // [nI][Kc]: this launch's sequences k0 .. k0 + Kc - 1
    int N, sdim, K, k0, Kc, nI;
};

// SD: s at compile time (20: the protein alphabet), 0 = the generic form; SEQ: sequences per thread.  Neither changes the order of
// a sequence's sum.
template <int SD, int SEQ>
__global__ __launch_bounds__(256) void k_energy_rows(const k_energy_rows_args a)
{
    constexpr int UB = SD == 20 ? 7 : 4;  // tile columns a wave has in flight (s = 20: its 21 columns in three rounds)
    extern __shared__ double lds_[];
    const int sdim = SD ? SD : a.sdim, s1 = sdim + 1, TD = ET * s1;
    double *tile = lds_;           // [TD columns][TD rows]
    double *gl = lds_ + TD * TD;   // [TD]: g of the row sites (0 at the gap rows)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int I = a.nI - 1 - (int)blockIdx.y;  // the long rows first
    const double *__restrict__ A = a.A;
    const size_t ld = a.ld;
    const int N = a.N;

    // the (up to two) tile rows this lane fills, whatever the tile: local row -> global row of A, or -1 (gap row, site beyond N)
    int grow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = lane + 64 * h;
        const int il = r / s1, ra = r - il * s1;
        grow[h] = (r < TD && ra < sdim && I * ET + il < N) ? (I * ET + il) * sdim + ra : -1;
        if (wave == 0 && r < TD) gl[r] = grow[h] >= 0 ? a.g[grow[h]] : 0.0;
    }

    // this thread's sequences: their row symbols as byte offsets into a tile column, kept over the whole walk
    const int kb = (int)blockIdx.x * (256 * SEQ) + t;  // + 256 u: within this launch's Kc sequences
    int roff[SEQ][ET];
    double acc[SEQ], accd[SEQ];
#pragma unroll
    for (int u = 0; u < SEQ; ++u) {
        const int kk = kb + 256 * u;
        const uint32_t w = kk < a.Kc ? a.Xg[(size_t)I * a.K + a.k0 + kk] : 0x01010101u * (uint32_t)sdim;
#pragma unroll
        for (int l = 0; l < ET; ++l) roff[u][l] = (l * s1 + (int)((w >> (8 * l)) & 0xffu)) * 8;
        acc[u] = 0.0;
        accd[u] = 0.0;
    }

    for (int J = 0; J <= I; ++J) {
        __syncthreads();  // (the previous tile has been read; first trip: gl is written)
        // (all loads of a round are issued before the first store: a load per column and trip was a latency per column)
        for (int cb0 = wave; cb0 < TD; cb0 += 4 * UB) {
            double v[UB][2];
#pragma unroll
            for (int b = 0; b < UB; ++b) {
                const int c = cb0 + 4 * b;
                const int jl = c / s1, ca = c - jl * s1;
                const bool cok = c < TD && ca < sdim && J * ET + jl < N;
                const size_t gcol = (size_t)((J * ET + jl) * sdim + ca) * ld;
#pragma unroll
                for (int h = 0; h < 2; ++h) v[b][h] = (cok && grow[h] >= 0) ? a.sign * A[gcol + grow[h]] : 0.0;
            }
#pragma unroll
            for (int b = 0; b < UB; ++b) {
                const int c = cb0 + 4 * b;
                if (c < TD) {
                    if (lane < TD) tile[c * TD + lane] = v[b][0];
                    if (lane + 64 < TD) tile[c * TD + lane + 64] = v[b][1];
                }
            }
        }
        __syncthreads();
        const char *tb = (const char *)tile;
        if (J < I) {
#pragma unroll
            for (int u = 0; u < SEQ; ++u) {
                const int kk = kb + 256 * u;
                const uint32_t w = kk < a.Kc ? a.Xg[(size_t)J * a.K + a.k0 + kk] : 0x01010101u * (uint32_t)sdim;
#pragma unroll
                for (int jl = 0; jl < ET; ++jl) {
                    const int cb = (jl * s1 + (int)((w >> (8 * jl)) & 0xffu)) * (TD * 8);
#pragma unroll
                    for (int il = 0; il < ET; ++il) acc[u] += *(const double *)(tb + cb + roff[u][il]);
                }
            }
        } else {
            // the diagonal tile: the pairs il > jl, and per site half its diagonal entry minus g
            const char *gb = (const char *)gl;
#pragma unroll
            for (int u = 0; u < SEQ; ++u) {
#pragma unroll
                for (int jl = 0; jl < ET; ++jl) {
                    const int cb = (roff[u][jl] >> 3) * (TD * 8);
#pragma unroll
                    for (int il = jl + 1; il < ET; ++il) acc[u] += *(const double *)(tb + cb + roff[u][il]);
                    accd[u] += 0.5 * *(const double *)(tb + cb + roff[u][jl]) - *(const double *)(gb + roff[u][jl]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < SEQ; ++u) {
        const int kk = kb + 256 * u;
        if (kk < a.Kc) a.part[(size_t)I * a.Kc + kk] = acc[u] + accd[u];
    }
}

__global__ __launch_bounds__(256) void k_energy_final(const double *__restrict__ part, int Kc, int nI, const double *c0,
                                                      double *__restrict__ E)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Kc) return;
    double acc = 0.0;
    for (int I = 0; I < nI; ++I) acc += part[(size_t)I * Kc + k];
    E[k] = acc + 0.5 * *c0;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
int gdca_energy_blocks(int Ns)
{
    return (Ns + ET - 1) / ET;
}

int gdca_energy_gblocks(int n)
{
    return (n + GT - 1) / GT;
}

// sequences one launch of k_energy_rows takes: a multiple of its workgroup's 256 x ESEQ_WIDE whose partials stay within ~256 MB
// (wanted > 0: option ENERGY_CHUNK, any count -- tests)
int gdca_energy_chunk(int N, int K, int wanted)
{
    const long long per = 256 * ESEQ_WIDE;
    long long kc = ((long long)256 << 20) / ((long long)gdca_energy_blocks(N) * 8) / per * per;
    if (kc < per) kc = per;
    if (wanted > 0) kc = wanted;
    return (int)(kc < K ? kc : K);
}

void gdca_launch_energy_pack(hipStream_t s, const int8_t *X, size_t stride, int Ns, int K, int q, uint32_t *Xg, gdca_dev_scalars *sc)
{
    GDCA_LAUNCH_DIRECT(k_energy_pack, dim3((K + 255) / 256, gdca_energy_blocks(Ns)), dim3(256), 0, s, X, stride, Ns, K, q, Xg, sc);
}

// g (n entries) and c0 (one) from the lower triangle of A (ld; sign -1: A holds -mJ); part: nb x (nb * 64) doubles, nb = gdca_energy_gblocks(n)
void gdca_launch_energy_g(hipStream_t s, const double *A, size_t ld, double sign, int n, const double *Pi, double *part, double *g,
                          double *c0)
{
    const int nb = gdca_energy_gblocks(n);
    const size_t ldp = (size_t)nb * GT;
    GDCA_LAUNCH_DIRECT(k_energy_gtile, dim3(nb, nb), dim3(256), 0, s, A, ld, n, Pi, part, ldp);
    GDCA_LAUNCH_DIRECT(k_energy_gfin, dim3((n + 255) / 256), dim3(256), 0, s, part, ldp, nb, n, sign, g);
    GDCA_LAUNCH_DIRECT(k_energy_c0, dim3(1), dim3(256), 0, s, Pi, g, n, c0);
}

// E[k0 .. k0 + Kc - 1] of the packed sequences Xg ([nI][K]); part: nI x Kc doubles.  An error: the dynamic LDS limit could not be
// raised for the tile (s >= 21), nothing was launched
hipError_t gdca_launch_energy_rows(hipStream_t s, const double *A, size_t ld, double sign, const double *g, const double *c0, const uint32_t *Xg,
                             int N, int sdim, int K, int k0, int Kc, double *part, double *E, int ncu)
{
    const int nI = gdca_energy_blocks(N);
    const k_energy_rows_args a{A, ld, sign, g, Xg, part, N, sdim, K, k0, Kc, nI};
    const int TD = ET * (sdim + 1);
    const size_t lds = (size_t)(TD * TD + TD) * sizeof(double);
    // eight sequences a thread -- or two, where eight would give fewer than two workgroups a compute unit (small N or K)
    const bool wide = gdca_wide_instance(Kc, 256 * ESEQ_WIDE, nI, ncu);
    const int per = 256 * (wide ? ESEQ_WIDE : ESEQ_NARROW);
    const dim3 grid((Kc + per - 1) / per, nI);
    void (*kern)(k_energy_rows_args) = sdim == 20 ? (wide ? k_energy_rows<20, ESEQ_WIDE> : k_energy_rows<20, ESEQ_NARROW>)
                                                  : (wide ? k_energy_rows<0, ESEQ_WIDE> : k_energy_rows<0, ESEQ_NARROW>);
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    GDCA_LAUNCH_DIRECT(kern, grid, dim3(256), lds, s, a);
    GDCA_LAUNCH_DIRECT(k_energy_final, dim3((Kc + 255) / 256), dim3(256), 0, s, part, Kc, nI, c0, E + k0);
    return hipSuccess;
}
