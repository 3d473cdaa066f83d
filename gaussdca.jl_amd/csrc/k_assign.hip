// The minimum-cost one-to-one assignment inside every block of a blocked f64 cost matrix (include/gdca.h, partner matching): species
// s owns the column-major kA_s x kB_s block at E + eoff[s]; min(kA_s, kB_s) pairs are matched at minimum total cost.
//
//   k_assign_blocks  one workgroup -- ONE WAVE -- a species.  Shortest augmenting paths (Jonker-Volgenant; the form of Crouse's
//                    rectangular algorithm): the SHORTER side's members are the rows, added one at a time; each addition grows a
//                    shortest-path tree over the columns from the new row until it reaches a free column, then shifts the potentials
//                    and flips the path.  Potentials u, v, the tentative distances minv, predecessors, both matchings and the
//                    visited flags live in LDS (40 B a member: 20 KB at GDCA_ASSIGN_MAX); the costs are read from the block where
//                    it lies (HBM / L2: a block of 32 x 32 is 8 KB).  The column scan of a step is spread over the lanes (column
//                    j = lane + 64 m), its minimum reduced by a fixed butterfly over (value, index): ties go to the lowest column.
//                    What steers the loops (the chosen column, its row) is made wave-uniform with readfirstlane, so every loop
//                    that holds a barrier is a scalar loop; with one wave a barrier costs nothing and orders the LDS traffic.
//                    The epilogue writes match and gap: gap[a] = min_{b' != match(a)} E[a, b'] - E[a, match(a)], ONE subtraction.
// ORDER-FIXED: no atomics; a species' result depends on its own block's bits alone (which optimum among equals: the one this scan
// order finds).  A step that finds no finite distance left (NaNs, infinities in the block) ends the whole species unmatched.
// Work: at most min(kA, kB) additions of at most max(kA, kB) steps of ceil(max / 64) column visits a lane -- k = 32: a few thousand
// dependent LDS round trips, tens of microseconds, all species side by side.
#include <limits.h>

#include "gdca_internal.h"
#include "gdca_launch.h"

struct k_assign_args {
    const double *E;
    const long long *eoff;   // [S + 1]
    const int *offA, *offB;  // [S + 1] each
    int *match;              // [KA]
    double *gap;             // [KA] or nullptr
    int kmax;                // the LDS arrays' length: >= every kA_s and kB_s
};

__global__ __launch_bounds__(64) void k_assign_blocks(const k_assign_args p)
{
    extern __shared__ double lds_[];
    const int km = p.kmax;
    double *u = lds_, *v = u + km, *minv = v + km;
    int *path = reinterpret_cast<int *>(minv + km), *row4col = path + km, *col4row = row4col + km, *seen = col4row + km;
    const int lane = threadIdx.x, sp = blockIdx.x;
    const int oa = p.offA[sp], ob = p.offB[sp];
    const int kA = p.offA[sp + 1] - oa, kB = p.offB[sp + 1] - ob;
    if (kA <= 0) return;
    const double *__restrict__ Eb = p.E + p.eoff[sp];
    const double inf = __builtin_inf();
    // rows = the shorter side: element (row i, column j) at Eb[i * sr + j * sc]
    const bool rows_a = kA <= kB;
    const int nr = rows_a ? kA : kB, nc = rows_a ? kB : kA;
    const long long sr = rows_a ? 1 : kA, sc = rows_a ? kA : 1;
    const int ncm = (nc + 63) >> 6;
    bool ok = kB > 0;

    for (int m = 0; m < ncm; ++m) {
        const int j = lane + 64 * m;
        if (j < nc) {
            v[j] = 0.0;
            row4col[j] = -1;
        }
        if (j < nr) {
            u[j] = 0.0;
            col4row[j] = -1;
        }
    }
    __syncthreads();
    for (int cur = 0; cur < nr && ok; ++cur) {
        for (int m = 0; m < ncm; ++m) {
            const int j = lane + 64 * m;
            if (j < nc) {
                minv[j] = inf;
                seen[j] = 0;
            }
        }
        __syncthreads();
        int i = cur, sink = -1;
        double minval = 0.0;
        while (sink < 0) {
            // relax the unvisited columns from row i, and the nearest of them
            const double ui = u[i];
            double best = inf;
            int bj = INT_MAX;
            for (int m = 0; m < ncm; ++m) {
                const int j = lane + 64 * m;
                if (j < nc && !seen[j]) {
                    const double r = ((minval + Eb[i * sr + j * sc]) - ui) - v[j];
                    double d = minv[j];
                    if (r < d) {
                        minv[j] = d = r;
                        path[j] = i;
                    }
                    if (d < best) {
                        best = d;
                        bj = j;
                    }
                }
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                const double ob_ = __shfl_xor(best, off);
                const int oj = __shfl_xor(bj, off);
                if (ob_ < best || (ob_ == best && oj < bj)) {
                    best = ob_;
                    bj = oj;
                }
            }
            const int js = __builtin_amdgcn_readfirstlane(bj);
            if (js >= nc) {  // nothing finite is left: a NaN or an infinity in the block
                ok = false;
                break;
            }
            minval = best;
            const int rj = __builtin_amdgcn_readfirstlane(row4col[js]);
            __syncthreads();  // (every lane has read seen[] and row4col[js])
            if (lane == 0) seen[js] = 1;
            __syncthreads();
            if (rj < 0)
                sink = js;
            else
                i = rj;
        }
        if (!ok) break;
        // the potentials: the new row by the path's length, the tree's rows and columns by what they were ahead of it
        for (int m = 0; m < ncm; ++m) {
            const int j = lane + 64 * m;
            if (j < nc && seen[j]) {
                const double d = minval - minv[j];
                v[j] -= d;
                const int r = row4col[j];
                if (r >= 0) u[r] += d;
            }
        }
        __syncthreads();
        if (lane == 0) {
            u[cur] += minval;
            int j = sink;
            for (int step = 0; step < nr; ++step) {  // (a path holds every row at most once)
                const int r = path[j];
                row4col[j] = r;
                const int jn = col4row[r];
                col4row[r] = j;
                j = jn;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }

    // match and gap of this species' sequences a
    const int nam = (kA + 63) >> 6;
    for (int m = 0; m < nam; ++m) {
        const int a = lane + 64 * m;
        if (a >= kA) continue;
        int mb = -1;
        if (ok) mb = rows_a ? col4row[a] : row4col[a];
        p.match[oa + a] = mb >= 0 ? ob + mb : -1;
        if (!p.gap) continue;
        double g = 0.0;
        if (mb >= 0) {
            double least = inf;
            for (int b = 0; b < kB; ++b) {
                const double e = Eb[a + (long long)kA * b];
                if (b != mb && e < least) least = e;
            }
            g = least - Eb[a + (long long)kA * mb];
        }
        p.gap[oa + a] = g;
    }
}

hipError_t gdca_launch_assign_blocks(hipStream_t s, const double *E, const long long *eoff, const int32_t *offA, const int32_t *offB, int S,
                                     int kmax, int32_t *match, double *gap)
{
    if (kmax < 1) kmax = 1;
    const size_t lds = (size_t)kmax * (3 * sizeof(double) + 4 * sizeof(int));
    const hipError_t e = gdca_raise_lds_limit(reinterpret_cast<const void *>(k_assign_blocks), lds);
    if (e != hipSuccess) return e;
    const k_assign_args a{E, eoff, offA, offB, match, gap, kmax};
    GDCA_LAUNCH_DIRECT(k_assign_blocks, dim3((unsigned)S), dim3(64), lds, s, a);
    return hipSuccess;
}
