// Double-mutant scan: the energy change of every DOUBLE substitution of K sequences under the fitted Gaussian model, without writing a
// mutant down.  With dE(x; i, b) of k_mutation.hip (what = delta) and K(i,b; j,c) = mJ[r(i,b), r(j,c)] (0 where b or c is the gap q),
// for sites i < j, a = x_i, a' = x_j and targets b (at i), c (at j):
//
//     E(x with i -> b, j -> c) - E(x) = dE(x; i, b) + dE(x; j, c) + eps(x; i, b; j, c)
//     eps = K(i,b; j,c) - K(i,a; j,c) - K(i,b; j,a') + K(i,a; j,a')
//
// (the two single changes each see the OTHER site at its wild type; eps puts the four couplings of the pair right).  eps, the
// epistasis, needs the s x s block (i, j) of mJ and the two wild-type symbols, nothing else.  The fixed f64 expressions, B[b,c] the
// block padded with a zero row and column for the gap:
//
//     eps[b,c] = (B[b,c] - B[a,c]) - (B[b,a'] - B[a,a'])           (exactly 0 for b == a and for c == a')
//     ddE[b,c] = (dE[i,b] + dE[j,c]) + eps[b,c]
//
// mJ is symmetric and only its lower triangle is read: block (i, j), i < j, is the rows r(j, .), columns r(i, .) of A -- element
// (b, c) at A[r(i,b) ld + r(j,c)], contiguous in c.  A fused run's ctx->A holds -mJ (sign = -1): every load is negated, which is exact,
// so both forms compute on the same values.
//   k_epi_tiles   a workgroup owns a TILE of 4 x 4 sites (site blocks TI <= TJ of the block lower triangle) and 64 sequences (lane =
//                 sequence; the sequence chunks are the fast grid index: the workgroups that share a tile run together); each of
//                 its four waves takes ONE column site j of the tile against the tile's four row sites i.  The tile's blocks go to
//                 LDS once as (4 (s + 1)) x (4 (s + 1)) doubles, the b index fastest, a zero row and column a site for the gap, the
//                 column stride odd (57 KB + 20 KB of staging at s = 20: two workgroups a compute unit; 145 KB at s = 30).  Per
//                 (sequence, block) a thread takes B[b,a'] - B[a,a'] and dE[i,b] for all b into registers (the per-lane LDS
//                 addresses: distinct symbols -> distinct banks, equal symbols broadcast), then walks the q^2 codes (b-1) + q (c-1)
//                 ascending -- c outside, b inside -- reading B[a,c] and dE[j,c] once a c and the column B[., c] at wave-uniform
//                 addresses (broadcasts, all of a column in flight before its arithmetic): four add/sub, a minimum, a multiply and an
//                 add for the sum of squares a code; the strict < for the minimiser once a column, and the winning column once
//                 more for its first b.  WRITES: an entry is 8 bytes and two sequences lie N^2 entries apart, so what a thread
//                 can make contiguous is the tile's four sites: it keeps its four results [i0 .. i0+3, j, k] in registers and
//                 stores them together (32 bytes), stages them in LDS, and after a barrier the wave of ROW site i stores the four
//                 mirror entries [j0 .. j0+3, i, k] together.  (One entry at a time, as first built, the partial lines left the L2
//                 before their neighbours arrived.)  The diagonal entries come from the diagonal tiles.
//   k_epi_list    one thread a record (k, i, b, j, c): checked (a bad record raises GDCA_BAD_MUTANT in sc->bad_symbol and indexes nothing), put
//                 into the orientation i < j, then the same two expressions on five gathers from A and two from dE.
// dE comes from k_mut_rows in a workspace of q N K doubles (gdca_api.hip).
// ORDER-FIXED: every entry is computed by ONE thread, the codes ascending, the minimiser the first code that reaches the minimum (what a
// walk with a strict < gives: +-0 compare equal, the first one's bits are returned); the sum of squares as one rounded
// product and one rounded sum a code (the library is built without contraction).  No floating-point atomics.  So an entry is the
// same bits from run to run, whatever K is, wherever x_k stands in the batch and whichever instance (s at compile time or not) runs.
#include "gdca_internal.h"
#include "gdca_launch.h"

#define DT 4     // sites per side of a tile (= symbols per packed dword)
#define ESEQ 64  // sequences a workgroup (lane = sequence); its four waves take one column site of the tile each

struct k_epi_args {
    const double *A;  // element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const uint32_t *Xg;  // [ceil(N / 4)][K]
    const double *D;     // [K][N][q]: dE
    double *Emin;        // [K][N][N], each may be nullptr
    int32_t *code;
    double *epi;
    int N, sdim, K;
    unsigned chunks;  // sequence chunks of ESEQ: workgroup w has chunk w % chunks of tile w / chunks
};

// SD: s at compile time (20: the protein alphabet), 0 = the generic form.  It changes no order.
template <int SD>
__global__ __launch_bounds__(256) void k_epi_tiles(const k_epi_args p)
{
    constexpr int NQ = SD ? SD + 1 : GDCA_MAXQ;  // targets a thread carries in registers
    extern __shared__ double lds_[];             // [DT (s + 1) columns c][LD], b fastest; behind it the staging of the mirror entries
    const int sdim = SD ? SD : p.sdim, q = sdim + 1, TW = DT * sdim, LW = DT * q, LD = LW + 1;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int N = p.N;
    double *stE = lds_ + (size_t)LW * LD;        // [il * DT + jl][lane] each
    double *stP = stE + DT * DT * ESEQ;
    int *stC = reinterpret_cast<int *>(stP + DT * DT * ESEQ);
    // tile -> (TI, TJ), TI <= TJ, the pairs of the block lower triangle row by row
    const long long tile = blockIdx.x / p.chunks;
    const unsigned chunk = blockIdx.x - (unsigned)tile * p.chunks;
    int TJ = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
    while ((long long)(TJ + 1) * (TJ + 2) / 2 <= tile) ++TJ;
    while ((long long)TJ * (TJ + 1) / 2 > tile) --TJ;
    const int TI = (int)(tile - (long long)TJ * (TJ + 1) / 2);
    const int si0 = TI * DT, sj0 = TJ * DT;

    for (int idx = t; idx < LW * LD; idx += 256) lds_[idx] = 0.0;
    __syncthreads();
    {
        const double *__restrict__ A = p.A;
        const size_t ld = p.ld;
        const double sign = p.sign;
        for (int idx = t; idx < TW * TW; idx += 256) {
            const int ii = idx / TW, jj = idx - ii * TW;  // (jj fastest: a row of the tile is contiguous)
            const int il = ii / sdim, jl = jj / sdim;
            const int i = si0 + il, j = sj0 + jl;
            if (i < j && j < N) lds_[(size_t)(jj + jl) * LD + ii + il] = sign * A[((size_t)si0 * sdim + ii) * ld + (size_t)sj0 * sdim + jj];
        }
    }
    __syncthreads();

    const long long kk = (long long)chunk * ESEQ + lane;
    const bool live = kk < p.K;
    const size_t k = live ? (size_t)kk : 0;
    const uint32_t wi = p.Xg[(size_t)TI * p.K + k], wj = p.Xg[(size_t)TJ * p.K + k];
    const size_t NN = (size_t)N * N;
    const double *__restrict__ Dk = p.D + k * (size_t)N * q;

    // ---- this wave's column site j = sj0 + wave against the tile's row sites: the entries [i, j, k], i ascending, are neighbours in memory
    {
        const int jl = wave, j = sj0 + jl;
        const int a2 = (int)((wj >> (8 * jl)) & 0xffu);
        const double *__restrict__ Dj = Dk + (size_t)j * q;
        const double *colA2 = lds_ + (size_t)(jl * q + a2) * LD;
        double rE[DT], rP[DT];
        int rC[DT];
#pragma unroll
        for (int il = 0; il < DT; ++il) {
            const int i = si0 + il;
            rE[il] = 0.0, rP[il] = 0.0, rC[il] = -1;  // (the diagonal entry's values)
            if (live && i < j && j < N) {             // (i < j, j < N: uniform in the wave)
                const int a = (int)((wi >> (8 * il)) & 0xffu);
                const double *__restrict__ Di = Dk + (size_t)i * q;
                const double baa = colA2[il * q + a];
                // Rb: B[b,a'] - B[a,a'];  Dm: dE[i,b], +inf at b == a -- an inadmissible target drops out of every minimum by itself
                double Rb[NQ], Dm[NQ];
#pragma unroll
                for (int b = 0; b < NQ; ++b) {
                    const bool ok = SD || b < q;
                    Rb[b] = ok ? colA2[il * q + b] - baa : 0.0;
                    Dm[b] = ok && b != a ? Di[b] : (double)INFINITY;
                }
                // The codes ascending, c outside: the minimum of a column is one v_min a code, the strict < against the best so far
                // once a column (the first column that holds the minimum wins, as in a walk over the codes one by one).
                double best = (double)INFINITY, ss = 0.0;
                int bc = -1;
                for (int c = 0; c < q; ++c) {
                    const double *col = lds_ + (size_t)(jl * q + c) * LD + il * q;
                    const double bac = col[a], djc = Dj[c];
                    // the whole column first, then the arithmetic: one LDS latency a column instead of one a pair of codes
                    double cb[NQ];
#pragma unroll
                    for (int b = 0; b < NQ; ++b) cb[b] = SD || b < q ? col[b] : 0.0;
                    __builtin_amdgcn_sched_barrier(0);
                    double m = (double)INFINITY;
#pragma unroll
                    for (int b = 0; b < NQ; ++b) {
                        if (SD || b < q) {  // (uniform; no break: the register arrays keep compile-time indices)
                            const double eps = (cb[b] - bac) - Rb[b];
                            const double dd = (Dm[b] + djc) + eps;
                            const double sq = eps * eps;
                            ss = ss + sq;
                            m = __builtin_fmin(m, dd);
                        }
                    }
                    if (c != a2 && m < best) {
                        best = m;
                        bc = c;
                    }
                }
                // ... and the first b of that column that reaches it: the same operations again, so the same bits
                int bcode = -1;
                if (bc >= 0) {
                    const double *col = lds_ + (size_t)(jl * q + bc) * LD + il * q;
                    const double bac = col[a], djc = Dj[bc];
                    int bb = 0;
                    double first = best;
#pragma unroll
                    for (int b = NQ - 1; b >= 0; --b) {
                        if (SD || b < q) {
                            const double dd = (Dm[b] + djc) + ((col[b] - bac) - Rb[b]);
                            if (dd == best) {
                                bb = b;
                                first = dd;
                            }
                        }
                    }
                    best = first;
                    bcode = bb + q * bc;
                }
                rE[il] = best, rP[il] = sqrt(ss), rC[il] = bcode;
            }
            stE[(il * DT + jl) * ESEQ + lane] = rE[il];
            stP[(il * DT + jl) * ESEQ + lane] = rP[il];
            stC[(il * DT + jl) * ESEQ + lane] = rC[il];
        }
        // [i, j, k] for the tile's i <= j: up to DT neighbouring entries a thread (the diagonal entry among them in a diagonal tile)
        if (live && j < N) {
            const size_t o = k * NN + (size_t)j * N + si0;
#pragma unroll
            for (int il = 0; il < DT; ++il) {
                if (si0 + il <= j) {
                    if (p.Emin) p.Emin[o + il] = rE[il];
                    if (p.code) p.code[o + il] = rC[il];
                    if (p.epi) p.epi[o + il] = rP[il];
                }
            }
        }
    }
    __syncthreads();
    // ---- the mirror entries [j, i, k]: this wave's ROW site i = si0 + wave, the tile's j > i ascending -- neighbours in memory again
    {
        const int il = wave, i = si0 + il;
        if (live && i < N) {
            const size_t o = k * NN + (size_t)i * N + sj0;
#pragma unroll
            for (int jl = 0; jl < DT; ++jl) {
                const int j = sj0 + jl;
                if (i < j && j < N) {
                    const int bcode = stC[(il * DT + jl) * ESEQ + lane];
                    if (p.Emin) p.Emin[o + jl] = stE[(il * DT + jl) * ESEQ + lane];
                    if (p.code) p.code[o + jl] = bcode < 0 ? -1 : bcode / q + q * (bcode % q);
                    if (p.epi) p.epi[o + jl] = stP[(il * DT + jl) * ESEQ + lane];
                }
            }
        }
    }
}

// One listed double mutant a thread: muts[5 r ..] = (k, i, b, j, c), sites 0-based, symbols 1..q.
__global__ __launch_bounds__(256) void k_epi_list(const double *__restrict__ A, size_t ld, double sign, const uint32_t *__restrict__ Xg,
                                                  const double *__restrict__ D, const int32_t *__restrict__ muts, long long L, int N,
                                                  int sdim, int K, double *__restrict__ out, gdca_dev_scalars *sc)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= L) return;
    const int32_t *m = muts + 5 * r;
    const int k = m[0], q = sdim + 1;
    int i = m[1], b = m[2], j = m[3], c = m[4];
    if (k < 0 || k >= K || i < 0 || i >= N || j < 0 || j >= N || i == j || b < 1 || b > q || c < 1 || c > q) {
        atomicOr(&sc->bad_symbol, GDCA_BAD_MUTANT);
        out[r] = 0.0;
        return;
    }
    if (i > j) {
        const int ti = i, tb = b;
        i = j, b = c;
        j = ti, c = tb;
    }
    --b, --c;  // (sdim: the gap)
    const int a = (int)((Xg[(size_t)(i >> 2) * K + k] >> (8 * (i & 3))) & 0xffu);
    const int a2 = (int)((Xg[(size_t)(j >> 2) * K + k] >> (8 * (j & 3))) & 0xffu);
    // B[u, v] of block (i, j), +0.0 where u or v is the gap
    auto B = [&](int u, int v) {
        return u < sdim && v < sdim ? sign * A[((size_t)i * sdim + u) * ld + (size_t)j * sdim + v] : 0.0;
    };
    const double *Dk = D + (size_t)k * N * q;
    const double eps = (B(b, c) - B(a, c)) - (B(b, a2) - B(a, a2));
    out[r] = (Dk[(size_t)i * q + b] + Dk[(size_t)j * q + c]) + eps;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
// Emin / code / epi [i + N (j + N k)] (each may be nullptr) of the K packed sequences Xg from the lower triangle of A (ld; sign -1: A
// holds -mJ) and D = dE [K][N][q].  generic: the form with s at run time also at s = 20 (the tests compare the two).  An error: the
// dynamic LDS limit could not be raised; nothing was launched.
hipError_t gdca_launch_double_mutant_scan(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, const double *D, int N,
                                          int sdim, int K, double *Emin, int32_t *code, double *epi, bool generic)
{
    const long long chunks = ((long long)K + ESEQ - 1) / ESEQ, nT = (N + DT - 1) / DT, tiles = nT * (nT + 1) / 2;
    if (chunks * tiles > GDCA_EPI_MAX_GROUPS) return hipErrorInvalidValue;  // (gdca_api.hip checks before: validate_double)
    const k_epi_args a{A, ld, sign, Xg, D, Emin, code, epi, N, sdim, K, (unsigned)chunks};
    const int q = sdim + 1, LW = DT * q;
    const size_t lds = (size_t)LW * (LW + 1) * sizeof(double) + (size_t)DT * DT * ESEQ * (2 * sizeof(double) + sizeof(int));
    void (*kern)(k_epi_args) = sdim == 20 && !generic ? k_epi_tiles<20> : k_epi_tiles<0>;
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    // (the sequence chunks run fastest: the workgroups that share a tile load it at the same time)
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)(chunks * tiles)), dim3(256), lds, s, a);
    return hipSuccess;
}

void gdca_launch_double_mutants(hipStream_t s, const double *A, size_t ld, double sign, const uint32_t *Xg, const double *D,
                                const int32_t *muts, long long L, int N, int sdim, int K, double *out, gdca_dev_scalars *sc)
{
    GDCA_LAUNCH_DIRECT(k_epi_list, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, s, A, ld, sign, Xg, D, muts, L, N, sdim, K, out, sc);
}
