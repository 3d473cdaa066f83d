// Pseudo-likelihood fit of the Potts model (W, 0) (plmDCA; include/gdca.h, "Pseudo-likelihood"): the conditional of a site given the
// rest of a sequence is the softmax of the mutation stage's site potentials, P(x_i = c | x_-i) = exp(-V(x; i, c)) / sum_c' exp(-V(x; i, c')),
// and the gradient of the weighted log pseudo-likelihood is the difference of the CONDITIONAL TALLIES and the family's frequencies, in
// the frequencies' own layout -- so the step and the fit read-out are k_bm.hip's as they stand.  The potentials come from
// k_mutation.hip (GDCA_MUT_POTENTIAL, [K][N][q], the gap last with V = +0.0); the kernels here are the rest:
//
//   k_plm_softmax   one thread a (k, i), all in f64, the table turned from V into p IN PLACE:
//                       m = min_c V_c (c = 1 .. q);  e_c = exp(m - V_c);  Zs = e_1 + .. + e_q added to +0.0 with c ascending;
//                       p_c = e_c / Zs;  l_ki = (V[x_ki] - m) + log(Zs)
//                   (the largest e_c is exp(0) = 1: Zs lies in [1, q], nothing overflows whatever V spans).  x_ki from the packed
//                   symbols of k_energy_pack (an illegal byte counts as the gap and is flagged there).
//   k_plm_nll_seq   nll_k = l_k0 + l_k1 + .. added to +0.0 with i ascending, by ONE thread a sequence.
//   k_plm_tally     the hot path.  Q[r, c] = sum_{k : x_k,site(c) = sym(c)} w_k p_k[r] and S[r] = sum_k w_k p_k[r].  k_mut_rows turned
//                   round: a workgroup is ONE wave, lane = row r (64 rows a row block), and owns one packed dword of column sites
//                   (PT = 4 sites) with its accumulator columns in LDS, (s + 1) x 64 doubles a site (10.75 KB at s = 20; 43 KB a
//                   wave: three waves a compute unit; 63.5 KB at s = 30: two).  Per sequence: ONE load of a = w_k p_k[r] (one rounded
//                   product; 512 contiguous bytes a wave, bar a site's gap entry every s; the loads of PU = 16 sequences are in
//                   flight at a time, issued a batch ahead), the dword of symbols wave-uniform (a scalar load), four conflict-free
//                   ds_read_b64 / add / ds_write_b64 into the columns the symbols select -- the gap's column is a dump that is never
//                   written out.  The four columns belong to four sites, so the four reads go out before the
//                   first write.  No barrier, no atomic.
//   k_plm_finish    Pij_c[r, c] = (Q[r, c] + Q[c, r]) / (2 Meff) outside the diagonal blocks (an IEEE addition commutes: symmetric to the
//                   bit), Pij_c[r, r] = Pi_c[r] = S[r] / Meff, +0.0 elsewhere inside a diagonal block: one division an entry.
//   k_plm_nll       nll = (sum_k w_k nll_k) / Meff: thread t of ONE workgroup the rounded products of k = t, t + 256, .. added to +0.0
//                   ascending, the 256 partials folded by the halving tree (t and t + 128, t and t + 64, ..), one division.
//   k_plm_check_w   a weight outside [0, 1] (or NaN): GDCA_BAD_WEIGHT in the device's flags.
// ORDER-FIXED: the sequences are cut into blocks of PLM_CHUNK (a context option).  Inside a block an entry's terms are added to +0.0 with k
// ascending (a sequence whose symbol does not select the entry adds nothing, not a zero); the blocks' partials are added to +0.0 with
// the block index ascending (Q and S start as +0.0, each block does Q = Q + partial).  Every entry has ONE owner, the launches of the
// slabs follow one another on the stream: the order depends on N, q, M and PLM_CHUNK alone.  No floating-point atomics.
#include "gdca_internal.h"
#include "gdca_launch.h"

#define PT 4  // column sites a wave of k_plm_tally owns (= symbols per packed dword)
#define PU 16  // sequences whose loads a wave of k_plm_tally keeps in flight

// ---- the conditionals ---------------------------------------------------------------------------------------------------------------------
// D [K][N][q]: V on entry, p on return; L [K][N]: l_ki
// QD: q at compile time (21: the protein alphabet -- the site's entries stay in registers, one read and one write of the table), 0 =
// the generic form (e_c parked in the table); the same operations in the same order, the same bits
template <int QD>
__global__ __launch_bounds__(256) void k_plm_softmax(double *__restrict__ D, const uint32_t *__restrict__ Xg, int N, int K, int q_,
                                                     double *__restrict__ L)
{
#pragma clang fp contract(off)
    const int q = QD ? QD : q_;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)N * K) return;
    const int k = (int)(at / N), i = (int)(at - (size_t)k * N);
    double *__restrict__ d = D + at * q;
    const int x = (int)((Xg[(size_t)(i >> 2) * K + k] >> (8 * (i & 3))) & 0xffu);  // 0 .. q - 1, the gap q - 1
    if (QD) {
        constexpr int QR = QD ? QD : 1;
        double v[QR];
#pragma unroll
        for (int c = 0; c < QR; ++c) v[c] = d[c];
        double m = v[0], vx = 0.0;
#pragma unroll
        for (int c = 1; c < QR; ++c) m = fmin(m, v[c]);
#pragma unroll
        for (int c = 0; c < QR; ++c) vx = c == x ? v[c] : vx;
        double Zs = 0.0;
#pragma unroll
        for (int c = 0; c < QR; ++c) {
            v[c] = exp(m - v[c]);
            Zs = Zs + v[c];
        }
#pragma unroll
        for (int c = 0; c < QR; ++c) d[c] = v[c] / Zs;
        L[at] = (vx - m) + log(Zs);
        return;
    }
    double m = d[0];
    for (int c = 1; c < q; ++c) m = fmin(m, d[c]);
    const double vx = d[x];
    double Zs = 0.0;
    for (int c = 0; c < q; ++c) {
        const double e = exp(m - d[c]);
        d[c] = e;
        Zs = Zs + e;
    }
    for (int c = 0; c < q; ++c) d[c] = d[c] / Zs;
    L[at] = (vx - m) + log(Zs);
}

__global__ __launch_bounds__(256) void k_plm_nll_seq(const double *__restrict__ L, int N, int K, double *__restrict__ nll_k)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double acc = 0.0;
    for (int i = 0; i < N; ++i) acc = acc + L[(size_t)k * N + i];
    nll_k[k] = acc;
}

// ---- the tally ----------------------------------------------------------------------------------------------------------------------------
struct k_plm_tally_args {
    const double *p;     // [K][N][q]
    const uint32_t *Xg;  // [ceil(N / 4)][K]
    const double *w;     // [K]
    double *Q;           // n x n, entry (r, c) at Q[c n + r]
    double *S;           // n
    int N, sdim, n, K, chunk;
};

template <int SD>
__global__ __launch_bounds__(64) void k_plm_tally(const k_plm_tally_args a)
{
#pragma clang fp contract(off)
    extern __shared__ double acc_[];  // [PT (s + 1) columns][64 rows]
    const int sdim = SD ? SD : a.sdim, s1 = sdim + 1, q = s1;
    const int lane = threadIdx.x, J = blockIdx.x;
    const int r = (int)blockIdx.y * 64 + lane;
    const bool rok = r < a.n;
    const size_t poff = rok ? (size_t)(r + r / sdim) : 0;  // (site i, symbol c) lies at i q + c = r + i
    const size_t seq = (size_t)a.N * q;
    const uint32_t *__restrict__ Xj = a.Xg + (size_t)J * a.K;
    const double *__restrict__ p = a.p;
    const double *__restrict__ w = a.w;
    double *col = acc_ + lane;

    for (int b0 = 0; b0 < a.K; b0 += a.chunk) {
        const int b1 = min(b0 + a.chunk, a.K);
        for (int cc = 0; cc < PT * s1; ++cc) col[cc * 64] = 0.0;
        double ps = 0.0;
        // PU sequences' loads are in flight at a time: a sequence's p lies N q doubles from the last one's, so every load is a miss of
        // its own, and one load a trip would leave the loop waiting a memory latency a sequence
        double pv[PU], wv[PU];
        uint32_t sv[PU];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const int kk = min(k0 + u, b1 - 1);  // (beyond the block: the last sequence read again, not used)
                pv[u] = p[(size_t)kk * seq + poff];
                wv[u] = w[kk];
                sv[u] = Xj[kk];
            }
        };
        fetch(b0);
        for (int k0 = b0; k0 < b1; k0 += PU) {
            double av[PU];
            uint32_t sy[PU];
#pragma unroll
            for (int u = 0; u < PU; ++u) av[u] = rok ? wv[u] * pv[u] : 0.0, sy[u] = sv[u];
            if (k0 + PU < b1) fetch(k0 + PU);  // (the next PU loads go out before this batch's columns are touched)
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                if (k0 + u >= b1) break;  // (wave-uniform)
                double *c0 = col + (0 * s1 + (int)(sy[u] & 0xffu)) * 64, *c1 = col + (1 * s1 + (int)((sy[u] >> 8) & 0xffu)) * 64,
                       *c2 = col + (2 * s1 + (int)((sy[u] >> 16) & 0xffu)) * 64, *c3 = col + (3 * s1 + (int)(sy[u] >> 24)) * 64;
                const double t0 = *c0, t1 = *c1, t2 = *c2, t3 = *c3;  // (four sites: four different columns)
                *c0 = t0 + av[u], *c1 = t1 + av[u], *c2 = t2 + av[u], *c3 = t3 + av[u];
                ps = ps + av[u];
            }
        }
        if (rok) {
            for (int l = 0; l < PT; ++l) {
                const int j = J * PT + l;
                if (j >= a.N) break;
                double *__restrict__ qc = a.Q + (size_t)j * sdim * a.n + r;
                for (int c = 0; c < sdim; ++c) qc[(size_t)c * a.n] = qc[(size_t)c * a.n] + col[(l * s1 + c) * 64];
            }
            if (J == 0) a.S[r] = a.S[r] + ps;
        }
    }
}

// ---- the finish ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_plm_finish(const double *__restrict__ Q, const double *__restrict__ S, int n, int sdim, double Meff,
                                                    double *__restrict__ Pi, double *__restrict__ Pij)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (r >= n) return;
    double out = 0.0;
    if (r / sdim != c / sdim) {
        const double two = 2.0 * Meff;  // (exact)
        const double sum = Q[(size_t)c * n + r] + Q[(size_t)r * n + c];
        out = sum / two;
    } else if (r == c) {
        out = S[r] / Meff;
        Pi[r] = out;
    }
    Pij[(size_t)c * n + r] = out;
}

__global__ __launch_bounds__(256) void k_plm_nll(const double *__restrict__ w, const double *__restrict__ nll_k, int M, double Meff,
                                                 double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int k = t; k < M; k += 256) {
        const double a = w[k] * nll_k[k];
        acc = acc + a;
    }
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) red[t] = red[t] + red[t + h];
        __syncthreads();
    }
    if (t == 0) *out = red[0] / Meff;
}

__global__ __launch_bounds__(256) void k_plm_check_w(const double *__restrict__ w, int M, gdca_dev_scalars *sc)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const double v = w[k];
    if (!(v >= 0.0 && v <= 1.0)) atomicOr(&sc->bad_symbol, GDCA_BAD_WEIGHT);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
void gdca_launch_plm_softmax(hipStream_t s, double *D, const uint32_t *Xg, int N, int K, int q, double *L, double *nll_k)
{
    const size_t total = (size_t)N * K;
    if (q == 21)
        GDCA_LAUNCH_DIRECT(k_plm_softmax<21>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, Xg, N, K, q, L);
    else
        GDCA_LAUNCH_DIRECT(k_plm_softmax<0>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, Xg, N, K, q, L);
    GDCA_LAUNCH_DIRECT(k_plm_nll_seq, dim3((K + 255) / 256), dim3(256), 0, s, L, N, K, nll_k);
}

// Q and S (+0.0 before the first slab) take the K sequences of a slab in: p [K][N][q], Xg the slab's packed symbols, w the slab's
// weights.  K but the last slab's is a multiple of chunk.  Returns what raising the dynamic LDS limit answered; nothing is launched on
// an error.
hipError_t gdca_launch_plm_tally(hipStream_t s, const double *p, const uint32_t *Xg, const double *w, int N, int sdim, int K, int chunk,
                                 double *Q, double *S)
{
    const int n = N * sdim;
    const k_plm_tally_args a{p, Xg, w, Q, S, N, sdim, n, K, chunk};
    const size_t lds = (size_t)PT * (sdim + 1) * 64 * sizeof(double);
    void (*kern)(k_plm_tally_args) = sdim == 20 ? k_plm_tally<20> : k_plm_tally<0>;
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    // (the column groups run fastest: the N / 4 waves that read the same 64 rows of p run side by side, so a row block's p comes from
    // HBM once an XCD and from L2 for the rest -- with the row blocks fastest every column group streamed the whole slab from HBM)
    GDCA_LAUNCH_DIRECT(kern, dim3((N + PT - 1) / PT, (n + 63) / 64), dim3(64), lds, s, a);
    return hipSuccess;
}

void gdca_launch_plm_finish(hipStream_t s, const double *Q, const double *S, int N, int sdim, double Meff, double *Pi, double *Pij)
{
    const int n = N * sdim;
    GDCA_LAUNCH_DIRECT(k_plm_finish, dim3((n + 255) / 256, n), dim3(256), 0, s, Q, S, n, sdim, Meff, Pi, Pij);
}

void gdca_launch_plm_nll(hipStream_t s, const double *w, const double *nll_k, int M, double Meff, double *out)
{
    GDCA_LAUNCH_DIRECT(k_plm_nll, dim3(1), dim3(256), 0, s, w, nll_k, M, Meff, out);
}

void gdca_launch_plm_check_weights(hipStream_t s, const double *w, int M, gdca_dev_scalars *sc)
{
    GDCA_LAUNCH_DIRECT(k_plm_check_w, dim3((M + 255) / 256), dim3(256), 0, s, w, M, sc);
}
