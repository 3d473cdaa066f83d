// Boltzmann-machine refinement: the Potts model the Metropolis chains (k_sample.hip) draw from, fitted to the one- and two-site
// frequencies of a family.  The model is a pair (W, 0) in mJ's layout (include/gdca.h, "Boltzmann-machine refinement"): W n x n,
// column-major, full symmetric, n = N s; off-diagonal blocks the couplings, W[r, r] = -2 h[r] the fields, the rest of a diagonal block
// +0.0.  One iteration is: sample (k_sample.hip), tally (k_tally.hip), read out, update -- the first two are the library's own stages,
// the kernels here are the rest:
//
//   k_bm_from_gaussian   the warm start: W from the lower triangle of mJ and g = mJ Pi (k_energy_gtile's g): off-diagonal blocks the bits
//                        of mJ (mirrored: both triangles the same bits), W[r, r] = mJ[r, r] - 2 g[r], the rest of a diagonal block +0.0.
//   k_bm_update          ONE pass over W in place, three reads and one write an entry (the HBM floor of 32 n^2 bytes): a thread owns
//                        VW consecutive rows (VW = 2: one 16-byte load a matrix, where n is even and the four pointers are aligned)
//                        of BM_COLS consecutive columns, every load of the tile issued before the first use.  The multiplier m of an
//                        entry (2 on the diagonal, 0 elsewhere in a diagonal block, 1 outside) needs the row's site once a thread and
//                        the column's site once a column (uniform).  Entry by entry, f64, no contraction:
//                            d = Pij_m - Pij_d;  g = m d;  m == 1 and lambda != 0: g = g - lambda W;  W = W + eta g.
//   k_bm_read_cols / k_bm_read_fin   the fit in three numbers: max |Pi_m - Pi_d|, and over the entries below the diagonal blocks
//                        (lower triangle) max |c_m - c_d| and the Pearson correlation of c_m and c_d, c = Pij[r, c] - Pi[r] Pi[c].
//                        Stage one: ONE workgroup a column c (the grid is n, whatever the device), thread t the rows r0 + t,
//                        r0 + t + 256, ... ascending (r0 the first row of the next site), then a fixed tree over the 256 threads.
//                        Stage two: one workgroup, thread t the columns t, t + 256, ... ascending, the same tree.
//   k_bm_accept          out = (sum of the chains' accepted proposals) / (K n_steps): integers summed exactly, one division.
//   k_bm_last_sample     X[:, k] <- the last sample of chain k.
//   k_bm_fill            a vector of equal doubles (the unit weights of the tally, the zero Pi of the container).
// ORDER-FIXED: the update and the warm start are entrywise; the read-out's sums are taken in the order above, which depends on n, N
// and q alone; maxima do not depend on an order.  No floating-point atomics.  The same bits from run to run.
#include "gdca_internal.h"
#include "gdca_launch.h"

#define BM_COLS 4  // columns a thread of k_bm_update carries

// ---- the warm start ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bm_from_gaussian(const double *__restrict__ mJ, const double *__restrict__ g, int n, int sdim,
                                                          double *__restrict__ W)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (r >= n) return;
    double w = 0.0;
    if (r / sdim != c / sdim) {
        const int lo = min(r, c), hi = max(r, c);
        w = mJ[(size_t)lo * n + hi];
    } else if (r == c) {
        w = mJ[(size_t)r * n + r] - 2.0 * g[r];
    }
    W[(size_t)c * n + r] = w;
}

// ---- the update ---------------------------------------------------------------------------------------------------------------------------
struct k_bm_update_args {
    double *W;
    const double *Pd, *Pm;  // Pij of the data and of the model, n x n
    int n, sdim;
    double eta, lambda;
};

__device__ __forceinline__ double bm_step(double w, double pd, double pm, double m, double eta, double lambda)
{
#pragma clang fp contract(off)
    const double d = pm - pd;
    double g = m * d;
    if (m == 1.0 && lambda != 0.0) {
        const double lw = lambda * w;
        g = g - lw;
    }
    const double e = eta * g;
    return w + e;
}

template <int VW>
__global__ __launch_bounds__(256) void k_bm_update(const k_bm_update_args p)
{
    const int n = p.n, sdim = p.sdim;
    const long long r0 = ((long long)blockIdx.x * 256 + threadIdx.x) * VW;
    if (r0 >= n) return;  // (n even where VW = 2: a thread's rows are all inside or all outside)
    const int c0 = (int)blockIdx.y * BM_COLS;
    double w[BM_COLS][VW], pd[BM_COLS][VW], pm[BM_COLS][VW];
#pragma unroll
    for (int u = 0; u < BM_COLS; ++u) {
        const int c = min(c0 + u, n - 1);  // (a column beyond the matrix: the last one read again, nothing stored)
        const size_t at = (size_t)c * n + (size_t)r0;
        if (VW == 2) {
            const double2 a = *reinterpret_cast<const double2 *>(p.W + at), b = *reinterpret_cast<const double2 *>(p.Pd + at),
                          d = *reinterpret_cast<const double2 *>(p.Pm + at);
            w[u][0] = a.x, w[u][VW - 1] = a.y, pd[u][0] = b.x, pd[u][VW - 1] = b.y, pm[u][0] = d.x, pm[u][VW - 1] = d.y;
        } else {
            w[u][0] = p.W[at], pd[u][0] = p.Pd[at], pm[u][0] = p.Pm[at];
        }
    }
    int site[VW];
#pragma unroll
    for (int v = 0; v < VW; ++v) site[v] = (int)((r0 + v) / sdim);
#pragma unroll
    for (int u = 0; u < BM_COLS; ++u) {
        const int c = c0 + u;
        if (c >= n) break;
        const int jc = c / sdim;
        double o[VW];
#pragma unroll
        for (int v = 0; v < VW; ++v) {
            const double m = r0 + v == c ? 2.0 : (site[v] == jc ? 0.0 : 1.0);
            o[v] = bm_step(w[u][v], pd[u][v], pm[u][v], m, p.eta, p.lambda);
        }
        const size_t at = (size_t)c * n + (size_t)r0;
        if (VW == 2)
            *reinterpret_cast<double2 *>(p.W + at) = make_double2(o[0], o[VW - 1]);
        else
            p.W[at] = o[0];
    }
}

// ---- the read-out -------------------------------------------------------------------------------------------------------------------------
#define BM_RED 6  // a column's partials: sum a, sum b, sum a a, sum a b, sum b b, max |a - b| (a = c_m, b = c_d)

// the fixed tree over the 256 threads' values: 128 + 128, 64 + 64, ... ; the result in red[0 .. BM_RED - 1][0]
__device__ __forceinline__ void bm_tree(double (*red)[256], const double *v, int t)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int f = 0; f < BM_RED; ++f) red[f][t] = v[f];
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int f = 0; f < BM_RED - 1; ++f) red[f][t] = red[f][t] + red[f][t + w];
            red[BM_RED - 1][t] = fmax(red[BM_RED - 1][t], red[BM_RED - 1][t + w]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bm_read_cols(const double *__restrict__ Pi_d, const double *__restrict__ Pij_d,
                                                      const double *__restrict__ Pi_m, const double *__restrict__ Pij_m, int n, int sdim,
                                                      double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double red[BM_RED][256];
    const int t = threadIdx.x, c = blockIdx.x;
    const int r0 = (c / sdim + 1) * sdim;  // the first row below the column's diagonal block
    const double pmc = Pi_m[c], pdc = Pi_d[c];
    const double *__restrict__ colm = Pij_m + (size_t)c * n, *__restrict__ cold = Pij_d + (size_t)c * n;
    double v[BM_RED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = r0 + t; r < n; r += 256) {
        const double qm = Pi_m[r] * pmc, qd = Pi_d[r] * pdc;
        const double a = colm[r] - qm, b = cold[r] - qd;
        const double aa = a * a, ab = a * b, bb = b * b;
        v[0] = v[0] + a, v[1] = v[1] + b, v[2] = v[2] + aa, v[3] = v[3] + ab, v[4] = v[4] + bb;
        v[5] = fmax(v[5], fabs(a - b));
    }
    bm_tree(red, v, t);
    if (t < BM_RED) part[(size_t)c * BM_RED + t] = red[t][0];
}

// out[0] = max |Pi_m - Pi_d|, out[1] = the columns' maximum, out[2] = the correlation from the columns' sums and the number of
// entries T (exact in f64); out[3] = +0.0 (zero3; the loop writes its own number there)
__global__ __launch_bounds__(256) void k_bm_read_fin(const double *__restrict__ part, const double *__restrict__ Pi_d,
                                                     const double *__restrict__ Pi_m, int n, double T, double *__restrict__ out, int zero3)
{
#pragma clang fp contract(off)
    __shared__ double red[BM_RED][256];
    const int t = threadIdx.x;
    double v[BM_RED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = t; c < n; c += 256) {
#pragma unroll
        for (int f = 0; f < BM_RED - 1; ++f) v[f] = v[f] + part[(size_t)c * BM_RED + f];
        v[5] = fmax(v[5], part[(size_t)c * BM_RED + 5]);
    }
    double m1 = 0.0;
    for (int r = t; r < n; r += 256) m1 = fmax(m1, fabs(Pi_m[r] - Pi_d[r]));
    bm_tree(red, v, t);
    __shared__ double mx[256];
    mx[t] = m1;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) mx[t] = fmax(mx[t], mx[t + w]);
        __syncthreads();
    }
    if (t == 0) {
        const double Sa = red[0][0], Sb = red[1][0], Saa = red[2][0], Sab = red[3][0], Sbb = red[4][0];
        const double tab = T * Sab, sab = Sa * Sb, taa = T * Saa, sa2 = Sa * Sa, tbb = T * Sbb, sb2 = Sb * Sb;
        const double num = tab - sab, va = taa - sa2, vb = tbb - sb2;
        const double den = sqrt(va) * sqrt(vb);
        out[0] = mx[0];
        out[1] = red[5][0];
        out[2] = num / den;
        if (zero3) out[3] = 0.0;
    }
}

// ---- what the loop adds -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bm_accept(const int32_t *__restrict__ accepted, int K, double denom, double *out)
{
    __shared__ unsigned long long red[256];
    const int t = threadIdx.x;
    unsigned long long acc = 0;
    for (int k = t; k < K; k += 256) acc += (unsigned long long)accepted[k];
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) *out = (double)red[0] / denom;
}

__global__ __launch_bounds__(256) void k_bm_last_sample(const int8_t *__restrict__ Xs, int N, int K, int n_samples, int8_t *__restrict__ X)
{
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)N * K) return;
    const size_t k = at / N, i = at - k * N;
    X[at] = Xs[(k * n_samples + (n_samples - 1)) * (size_t)N + i];
}

__global__ __launch_bounds__(256) void k_bm_fill(double *__restrict__ v, size_t count, double value)
{
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at < count) v[at] = value;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
void gdca_launch_bm_from_gaussian(hipStream_t s, const double *mJ, const double *g, int N, int sdim, double *W)
{
    const int n = N * sdim;
    GDCA_LAUNCH_DIRECT(k_bm_from_gaussian, dim3((n + 255) / 256, n), dim3(256), 0, s, mJ, g, n, sdim, W);
}

void gdca_launch_bm_update(hipStream_t s, double *W, const double *Pij_d, const double *Pij_m, int N, int sdim, double eta, double lambda)
{
    const int n = N * sdim;
    const k_bm_update_args a{W, Pij_d, Pij_m, n, sdim, eta, lambda};
    const bool wide = n % 2 == 0 && (((uintptr_t)W | (uintptr_t)Pij_d | (uintptr_t)Pij_m) & 15) == 0;
    const int rows = wide ? 512 : 256;
    const dim3 grid((n + rows - 1) / rows, (n + BM_COLS - 1) / BM_COLS);
    if (wide)
        GDCA_LAUNCH_DIRECT(k_bm_update<2>, grid, dim3(256), 0, s, a);
    else
        GDCA_LAUNCH_DIRECT(k_bm_update<1>, grid, dim3(256), 0, s, a);
}

size_t gdca_bm_readout_bytes(int n)
{
    return (size_t)n * BM_RED * sizeof(double);
}

void gdca_launch_bm_readout(hipStream_t s, const double *Pi_d, const double *Pij_d, const double *Pi_m, const double *Pij_m, int N, int sdim,
                            double *part, double *out, bool zero3)
{
    const int n = N * sdim;
    const double T = (double)((long long)sdim * sdim * ((long long)N * (N - 1) / 2));  // (below 2^53: exact)
    GDCA_LAUNCH_DIRECT(k_bm_read_cols, dim3(n), dim3(256), 0, s, Pi_d, Pij_d, Pi_m, Pij_m, n, sdim, part);
    GDCA_LAUNCH_DIRECT(k_bm_read_fin, dim3(1), dim3(256), 0, s, part, Pi_d, Pi_m, n, T, out, zero3 ? 1 : 0);
}

void gdca_launch_bm_accept(hipStream_t s, const int32_t *accepted, int K, long long n_steps, double *out)
{
    GDCA_LAUNCH_DIRECT(k_bm_accept, dim3(1), dim3(256), 0, s, accepted, K, (double)((long long)K * n_steps), out);
}

void gdca_launch_bm_last_sample(hipStream_t s, const int8_t *Xs, int N, int K, int n_samples, int8_t *X)
{
    const size_t total = (size_t)N * K;
    GDCA_LAUNCH_DIRECT(k_bm_last_sample, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Xs, N, K, n_samples, X);
}

void gdca_launch_bm_fill(hipStream_t s, double *v, size_t count, double value)
{
    if (!count) return;
    GDCA_LAUNCH_DIRECT(k_bm_fill, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, v, count, value);
}
