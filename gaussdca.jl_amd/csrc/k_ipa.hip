// The glue of iterative partner matching (include/gdca.h, "iterative partner matching"): between two rounds of fit and
// match the loop ranks the matches by confidence, selects the next training set and writes the next training alignment from the two
// pools -- all three here, so that a round hands the host a few scalars and nothing else.
//
//   selection   k_ipa_keys      key[a] = the ranking's 64-bit key of gap[a] (gdca_rank_key: descending under isless, NaN first, 0.0 before
//                               -0.0) for a candidate (match[a] >= 0), the largest key for everybody else; val[a] = a
//               the ranking's eight stable radix passes (k_rank.hip, gdca_launch_sort_pairs): equal keys stay in ascending a
//               k_ipa_flag      flag[val[r]] = r < n_take and val[r] is a candidate: a flag per a by rank
//               k_ipa_compact   one workgroup: an exclusive scan of the flags (thread t owns a fixed stretch of a, then a fixed scan over
//                               the 1024 counts), the selected a written in ascending order, -1 behind them; the counts for the host
//   concat      k_ipa_concat    one thread a byte of the new columns: column col0 + t = XA[:, selA[t]] over XB[:, selB[t]], consecutive
//                               threads store consecutive bytes; an index outside its pool raises GDCA_BAD_INDEX in sc->bad_symbol and its column is
//                               left alone (nothing is read out of bounds)
//   a round's   k_ipa_round     one workgroup: the total cost sum_a E[a, match[a]] in f64 -- thread t takes a = t, t + 1024, ... in
//   figures                     ascending order, then a fixed binary tree, as k_logdet does -- and the number of a whose match changed
//               k_ipa_publish   the round's match / gap into the caller's arrays, its trace rows and the copy the next round compares with
//
// No floating-point atomics and no order-dependent integer ones: every result is a function of the input bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gdca_internal.h"
#include "gdca_launch.h"

#define IPA_THREADS 1024

namespace {

__global__ __launch_bounds__(256) void k_ipa_keys(const int32_t *__restrict__ match, const double *__restrict__ gap, int KA, uint64_t *__restrict__ key,
                                                  uint32_t *__restrict__ val)
{
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= (size_t)KA) return;
    // (no candidate's key is ~0: gdca_rank_key gives that to no double)
    key[a] = match[a] >= 0 ? gdca_rank_key(gap[a]) : ~0ull;
    val[a] = (uint32_t)a;
}

__global__ __launch_bounds__(256) void k_ipa_flag(const uint32_t *__restrict__ val, const int32_t *__restrict__ match, int KA, int n_take,
                                                  int32_t *__restrict__ flag)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)KA) return;
    const uint32_t a = val[r];
    if (a < (uint32_t)KA) flag[a] = ((long long)r < (long long)n_take && match[a] >= 0) ? 1 : 0;
}

__global__ __launch_bounds__(IPA_THREADS) void k_ipa_compact(const int32_t *__restrict__ flag, const int32_t *__restrict__ match, int KA,
                                                             int32_t *__restrict__ sel, gdca_ipa_counts *__restrict__ out)
{
    __shared__ int scan[IPA_THREADS], cand[IPA_THREADS];
    const int tid = (int)threadIdx.x;
    const long long per = ((long long)KA + IPA_THREADS - 1) / IPA_THREADS;
    const long long lo = tid * per < KA ? tid * per : KA, hi = lo + per < KA ? lo + per : KA;
    int c = 0, m = 0;
    for (long long a = lo; a < hi; ++a) {
        c += flag[a];
        m += match[a] >= 0 ? 1 : 0;
    }
    scan[tid] = c;
    cand[tid] = m;
    __syncthreads();
    for (int off = 1; off < IPA_THREADS; off <<= 1) {  // inclusive scans of both over the threads
        const int v = tid >= off ? scan[tid - off] : 0, w = tid >= off ? cand[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        cand[tid] += w;
        __syncthreads();
    }
    const int total = scan[IPA_THREADS - 1];
    long long at = scan[tid] - c;
    for (long long a = lo; a < hi; ++a)
        if (flag[a]) sel[at++] = (int32_t)a;
    for (long long t = (long long)total + tid; t < KA; t += IPA_THREADS) sel[t] = -1;
    if (tid == 0) {
        out->ncand = cand[IPA_THREADS - 1];
        out->n_sel = total;
    }
}

__global__ __launch_bounds__(256) void k_ipa_concat(const int8_t *__restrict__ XA, int KA, const int8_t *__restrict__ XB, int KB, int N, int split,
                                                    const int32_t *__restrict__ selA, const int32_t *__restrict__ selB,
                                                    const int32_t *__restrict__ viaB, int n_sel, int8_t *__restrict__ Z, size_t col0,
                                                    gdca_dev_scalars *sc)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n_sel * (size_t)N) return;
    const size_t t = e / (size_t)N;
    const int i = (int)(e - t * (size_t)N);
    const int32_t a = selA[t];
    const bool a_ok = a >= 0 && a < KA;
    const int32_t b = viaB ? (a_ok ? viaB[a] : -1) : selB[t];
    if (!a_ok || b < 0 || b >= KB) {
        if (i == 0) atomicOr(&sc->bad_symbol, GDCA_BAD_INDEX);
        return;
    }
    Z[(col0 + t) * (size_t)N + i] = i < split ? XA[(size_t)a * split + i] : XB[(size_t)b * (N - split) + (i - split)];
}

__global__ __launch_bounds__(IPA_THREADS) void k_ipa_round(const double *__restrict__ E, const long long *__restrict__ eoff,
                                                           const int32_t *__restrict__ offA, const int32_t *__restrict__ offB,
                                                           const int32_t *__restrict__ spA, const int32_t *__restrict__ match,
                                                           const int32_t *__restrict__ prev, int KA, gdca_ipa_counts *__restrict__ out)
{
    __shared__ double part[IPA_THREADS];
    __shared__ int chg[IPA_THREADS];
    const int tid = (int)threadIdx.x;
    double acc = 0.0;
    int ch = 0;
    for (long long a = tid; a < KA; a += IPA_THREADS) {
        const int32_t b = match[a];
        if (b >= 0) {
            const int s = spA[a];
            const int32_t a0 = offA[s], b0 = offB[s];
            if (b >= b0 && b < offB[s + 1]) acc += E[eoff[s] + (a - a0) + (long long)(offA[s + 1] - a0) * (b - b0)];
        }
        ch += prev ? (b != prev[a] ? 1 : 0) : (b >= 0 ? 1 : 0);
    }
    part[tid] = acc;
    chg[tid] = ch;
    __syncthreads();
#pragma unroll
    for (int h = IPA_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            part[tid] += part[tid + h];
            chg[tid] += chg[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out->cost = part[0];
        out->n_changed = chg[0];
    }
}

// a completed round's match / gap where they are wanted, in one launch: the copy the next round's figures compare with, the caller's
// arrays, the caller's trace rows (any of the last three may be nullptr)
__global__ __launch_bounds__(256) void k_ipa_publish(const int32_t *__restrict__ match, const double *__restrict__ gap, int KA,
                                                     int32_t *__restrict__ prev, int32_t *__restrict__ match_out, double *__restrict__ gap_out,
                                                     int32_t *__restrict__ match_row, double *__restrict__ gap_row)
{
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= (size_t)KA) return;
    const int32_t b = match[a];
    const double g = gap[a];
    prev[a] = b;
    match_out[a] = b;
    if (gap_out) gap_out[a] = g;
    if (match_row) match_row[a] = b;
    if (gap_row) gap_row[a] = g;
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t gdca_ipa_select_ws_bytes(int KA)
{
    const size_t n = (size_t)KA;
    return 2 * up256(n * 8) + 2 * up256(n * 4) + up256(gdca_sort_hist_words(n) * 4) + up256(n * 4);
}

void gdca_launch_ipa_select(hipStream_t s, const int32_t *match, const double *gap, int KA, int n_take, void *ws, int32_t *sel, gdca_ipa_counts *out)
{
    const size_t n = (size_t)KA;
    char *p = (char *)ws;
    uint64_t *key[2];
    uint32_t *val[2];
    key[0] = (uint64_t *)p, p += up256(n * 8);
    key[1] = (uint64_t *)p, p += up256(n * 8);
    val[0] = (uint32_t *)p, p += up256(n * 4);
    val[1] = (uint32_t *)p, p += up256(n * 4);
    uint32_t *hist = (uint32_t *)p;
    p += up256(gdca_sort_hist_words(n) * 4);
    int32_t *flag = (int32_t *)p;
    const dim3 grid((unsigned)((n + 255) / 256));
    GDCA_LAUNCH_DIRECT(k_ipa_keys, grid, dim3(256), 0, s, match, gap, KA, key[0], val[0]);
    gdca_launch_sort_pairs(s, key, val, hist, n);
    GDCA_LAUNCH_DIRECT(k_ipa_flag, grid, dim3(256), 0, s, val[0], match, KA, n_take, flag);
    GDCA_LAUNCH_DIRECT(k_ipa_compact, dim3(1), dim3(IPA_THREADS), 0, s, flag, match, KA, sel, out);
}

void gdca_launch_ipa_concat(hipStream_t s, const int8_t *XA, int KA, const int8_t *XB, int KB, int N, int split, const int32_t *selA,
                            const int32_t *selB, const int32_t *viaB, int n_sel, int8_t *Z, size_t col0, gdca_dev_scalars *sc)
{
    const size_t bytes = (size_t)n_sel * (size_t)N;
    if (!bytes) return;
    GDCA_LAUNCH_DIRECT(k_ipa_concat, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, s, XA, KA, XB, KB, N, split, selA, selB, viaB, n_sel, Z,
                       col0, sc);
}

void gdca_launch_ipa_round(hipStream_t s, const double *E, const long long *eoff, const int32_t *offA, const int32_t *offB, const int32_t *spA,
                           const int32_t *match, const int32_t *prev, int KA, gdca_ipa_counts *out)
{
    GDCA_LAUNCH_DIRECT(k_ipa_round, dim3(1), dim3(IPA_THREADS), 0, s, E, eoff, offA, offB, spA, match, prev, KA, out);
}

void gdca_launch_ipa_publish(hipStream_t s, const int32_t *match, const double *gap, int KA, int32_t *prev, int32_t *match_out, double *gap_out,
                             int32_t *match_row, double *gap_row)
{
    GDCA_LAUNCH_DIRECT(k_ipa_publish, dim3((unsigned)(((size_t)KA + 255) / 256)), dim3(256), 0, s, match, gap, KA, prev, match_out, gap_out,
                       match_row, gap_row);
}
