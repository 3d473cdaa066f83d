// Mutation scan: the energy change of every single substitution of K sequences under the fitted Gaussian model -- the mutational
// landscape people compare with deep mutational scans.  With E(x) = 1/2 (x - Pi)' mJ (x - Pi) of k_energy.hip, one-hot x, g = mJ Pi,
// r(i, c) = i s + c - 1 and d = x - Pi, setting site i from symbol a to b adds delta = e_b - e_a (a unit vector less for a gap):
//
//     E(x + delta) - E(x) = delta' mJ d + 1/2 delta' mJ delta
//                         = (mJ x - g)[r(i,b)] - (mJ x - g)[r(i,a)] + 1/2 (mJ[bb] + mJ[aa]) - mJ[ab]
//
// and (mJ x)[r(i,c)] holds the site's own term mJ[r(i,c), r(i,a)]: taking it out of both cancels the - mJ[ab] and turns the + 1/2 mJ[aa]
// into - 1/2 mJ[aa].  So with the SITE POTENTIAL
//
//     V(x; i, c) = sum_{j != i, x_j no gap} mJ[r(i,c), r(j,x_j)] + 1/2 mJ[r(i,c), r(i,c)] - g[r(i,c)],    V(x; i, gap) = +0.0
//
// the change is dE(x; i, b) = V(x; i, b) - V(x; i, x_i): one row block of mJ applied to the wild type, N gathers an entry where the
// explicit mutant costs N^2 / 2, and no mutant is ever written down.
//
// mJ is symmetric and only its lower triangle is read (ctx->A of the fused path holds -mJ there: `sign` = -1, ld = n_pad; the operator
// form: sign +1, ld = n), but V needs every row on both sides of the diagonal:
//   k_mut_rows   a workgroup owns a ROW BLOCK of floor(64 / s) whole sites (lane = row; 60 of 64 lanes at s = 20) and 4 x AU sequences;
//                it walks ALL column tiles J (4 sites = one dword of k_energy_pack's symbols): a tile below the block is read as it lies
//                (lane = row: a column segment is contiguous), a tile above it transposed (lane = column: a row segment of the mirrored
//                tile is contiguous), the one or two that meet the diagonal element by element, the own site's s x s block as zeros.
//                The tile sits in LDS as 4 (s + 1) columns (a zero column per site: the gap) of 65 doubles (43 KB at s = 20, 63 KB at
//                s = 30: two workgroups a compute unit; 65: the transposed stores do not pile up on one bank), the next tile's loads are
//                in flight in registers while this one is gathered.  Each wave adds, for each of its AU sequences, the four columns the
//                sequence's symbols select (lane = row, the column wave-uniform: conflict-free ds_read_b64).  Epilogue: 1/2 diag - g,
//                and, `what` = delta, ONE subtraction of the potential of the wild-type symbol, which lives in a lane of the same wave
//                (a row block holds whole sites); the gap target (column q) is 0 - that.
// The symbol check and the packed symbols are k_energy_pack's, g is k_energy_gtile's: an illegal byte is flagged before anything
// is indexed with it and counts as a gap.  No buffer grows with K but the packed symbols (N bytes a sequence), so nothing is chunked.
// ORDER-FIXED: V[k, i, c] is summed by ONE thread over the tiles J ascending, the sites ascending inside a tile (a gap and the own site
// adding an exact zero in their place), then + (1/2 diag - g).  No floating-point atomics.  So D[k, i, :] is the same bits from run to
// run, whatever K is, wherever x_k stands in the batch and whichever instance (s at compile time or not, AU) runs.
#include "gdca_internal.h"
#include "gdca_launch.h"

#define MT 4          // sites per column tile (= symbols per packed dword)
#define MLD 65        // doubles per tile column in LDS (64 rows + 1)
#define MAU_WIDE 32   // sequences per wave ...
#define MAU_NARROW 4  // ... and where that would leave compute units without a workgroup

struct k_mut_args {
    const double *A;  // element (row, col), row >= col, at A[col * ld + row]
    size_t ld;
    double sign;
    const double *g;
    const uint32_t *Xg;  // [ceil(N / 4)][K]
    double *D;           // [K][N][q]
    int N, sdim, n, K, what;
};

// SD: s at compile time (20: the protein alphabet), 0 = the generic form; AU: sequences per wave.  Neither changes the order of a sum.
template <int SD, int AU>
__global__ __launch_bounds__(256) void k_mut_rows(const k_mut_args p)
{
    constexpr int NV = SD ? SD : GDCA_MAXQ - 1;  // tile elements a thread carries: 64 rows x 4 s columns / 256
    extern __shared__ double lds_[];             // [MT (s + 1) columns][MLD]
    const int sdim = SD ? SD : p.sdim, s1 = sdim + 1, TW = MT * sdim;
    const int spb = 64 / sdim;  // sites per row block
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int site0 = (int)blockIdx.y * spb;
    const int il = lane / sdim, ca = lane - il * sdim;
    const int isite = site0 + il;
    const bool rok = il < spb && isite < p.N;
    const int row = rok ? isite * sdim + ca : 0;
    const int row0 = site0 * sdim;
    const int nrows = min(spb, p.N - site0) * sdim;
    const double *__restrict__ A = p.A;
    const size_t ld = p.ld;
    const double sign = p.sign;
    const int kb = (int)blockIdx.x * (4 * AU) + wave * AU;  // this wave's first sequence
    const uint32_t gapw = 0x01010101u * (uint32_t)sdim;

    double acc[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) acc[u] = 0.0;
    // the gap columns stay zero over the whole walk
    for (int idx = t; idx < MT * MLD; idx += 256) {
        const int jl = idx / MLD;
        lds_[(jl * s1 + sdim) * MLD + (idx - jl * MLD)] = 0.0;
    }

    const int nJ = (p.N + MT - 1) / MT;
    // tile J lies wholly above the row block: all its column sites beyond the block's last site
    auto above = [&](int J) { return J * MT > site0 + spb - 1; };
    double v[NV];
    auto fetch = [&](int J) {
        const int col0 = J * TW;
        if (!above(J)) {
            // lane = row, this wave's columns wave, wave + 4, ...: below the diagonal as it lies, above it mirrored
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const int tt = wave + 4 * m;
                const int csite = J * MT + tt / sdim, gcol = col0 + tt;
                const bool ok = rok && tt < TW && csite < p.N && csite != isite;
                const int lo = min(row, gcol), hi = max(row, gcol);
                v[m] = ok ? sign * A[(size_t)lo * ld + hi] : 0.0;
            }
        } else {
            // lane = column: row r of the tile is a contiguous piece of column row0 + r of the lower triangle
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const int idx = t + 256 * m;
                const int r = idx / TW, tt = idx - r * TW;
                const bool ok = r < nrows && col0 + tt < p.n;
                v[m] = ok ? sign * A[(size_t)(row0 + r) * ld + col0 + tt] : 0.0;
            }
        }
    };
    auto stash = [&](int J) {
        if (!above(J)) {
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const int tt = wave + 4 * m;
                if (tt < TW) lds_[(tt + tt / sdim) * MLD + lane] = v[m];
            }
        } else {
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const int idx = t + 256 * m;
                const int r = idx / TW, tt = idx - r * TW;
                if (r < 64) lds_[(tt + tt / sdim) * MLD + r] = v[m];
            }
        }
    };

    fetch(0);
    for (int J = 0; J < nJ; ++J) {
        __syncthreads();  // (the previous tile has been read; first trip: the gap columns are written)
        stash(J);
        // the symbols of this wave's sequences at the tile's four sites: lane u holds sequence u's
        uint32_t w = gapw;
        if (lane < AU && kb + lane < p.K) w = p.Xg[(size_t)J * p.K + kb + lane];
        __syncthreads();
        if (J + 1 < nJ) fetch(J + 1);
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const uint32_t wu = (uint32_t)__builtin_amdgcn_readlane((int)w, u);
#pragma unroll
            for (int l = 0; l < MT; ++l) acc[u] += lds_[(l * s1 + (int)((wu >> (8 * l)) & 0xffu)) * MLD + lane];
        }
    }

    // V = acc + (1/2 diag - g); delta: minus the potential of the wild-type symbol, held by a lane of this wave
    const double h = rok ? 0.5 * (sign * A[(size_t)row * ld + row]) - p.g[row] : 0.0;
    const int q = sdim + 1;
#pragma unroll
    for (int u = 0; u < AU; ++u) {
        const int kk = kb + u;  // (wave-uniform)
        if (kk >= p.K) break;
        const double V = acc[u] + h;
        double out = V, gout = 0.0;
        if (p.what == GDCA_MUT_DELTA) {
            int sym = sdim;
            if (rok) sym = (int)((p.Xg[(size_t)(isite >> 2) * p.K + kk] >> (8 * (isite & 3))) & 0xffu);
            const double vr = __shfl(V, il * sdim + (sym < sdim ? sym : 0), 64);
            const double ref = sym < sdim ? vr : 0.0;
            out = V - ref;
            gout = 0.0 - ref;
        }
        if (rok) {
            double *d = p.D + ((size_t)kk * p.N + isite) * q;
            d[ca] = out;
            if (ca == sdim - 1) d[sdim] = gout;
        }
    }
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------
// D[(b - 1) + q (i + N k)] of the K packed sequences Xg ([gdca_energy_blocks(N)][K]) from the lower triangle of A (ld; sign -1: A holds
// -mJ) and g = mJ Pi.  Returns what raising the dynamic LDS limit answered (s >= 23: the tile is beyond 48 KB); nothing is launched on an error.
hipError_t gdca_launch_mutation_scan(hipStream_t s, const double *A, size_t ld, double sign, const double *g, const uint32_t *Xg, int N, int sdim,
                               int K, int what, double *D, int ncu)
{
    const k_mut_args a{A, ld, sign, g, Xg, D, N, sdim, N * sdim, K, what};
    const int spb = 64 / sdim, nR = (N + spb - 1) / spb;
    // 128 sequences a workgroup -- or 16, where 128 would give fewer than two workgroups a compute unit
    const bool wide = gdca_wide_instance(K, 4 * MAU_WIDE, nR, ncu);
    const int per = 4 * (wide ? MAU_WIDE : MAU_NARROW);
    const size_t lds = (size_t)MT * (sdim + 1) * MLD * sizeof(double);
    void (*kern)(k_mut_args) = sdim == 20 ? (wide ? k_mut_rows<20, MAU_WIDE> : k_mut_rows<20, MAU_NARROW>)
                                          : (wide ? k_mut_rows<0, MAU_WIDE> : k_mut_rows<0, MAU_NARROW>);
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    // (the sequence chunks run fastest: the workgroups that share a row block walk the same tiles at the same time)
    GDCA_LAUNCH_DIRECT(kern, dim3((unsigned)(((long long)K + per - 1) / per), nR), dim3(256), lds, s, a);
    return hipSuccess;
}
