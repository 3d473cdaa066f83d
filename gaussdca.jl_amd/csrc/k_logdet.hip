// log det C from the pivots of the elimination, and the epilogue that turns energies into log-likelihoods (include/gdca.h, "Log-likelihoods";
// DESIGN.md 3.6a).
//
// The block sweep (k_inverse.hip, pivot_chain) and the Cholesky fallback (k_chol_diag) leave the n_pad pivots d_i of symmetric
// elimination without pivoting -- the squares of the Cholesky diagonal -- in one vector of the inverse's workspace, so
//       log det C = sum_{i < n} log d_i
// costs one pass over n doubles behind the inverse: no second factorisation, nothing of the n^3 work.
#include <math.h>

#include "gdca_internal.h"
#include "gdca_launch.h"

#define LOGDET_THREADS 1024

// sc->logdet = sum_{i < n_real} log(piv[i]): thread t takes i = t, t + 1024, ... in ascending order, then a fixed binary tree over the 1024
// partial sums -- the same bits whenever the pivots are the same bits, whatever else runs.  One workgroup of 1024: an f64 logarithm is
// some hundred instructions, and at n = 10 000 a thread has ten of them (with 256 threads the kernel took 24 us there).  The padding
// rows (identity: pivot 1) are not read.  Quiet NaN where the inverse did not end well (sc->info != 0: a non-positive pivot, or a
// launch the sweep's watchdog ended).
struct k_logdet_args {
    const double *piv;
    int n_real;
    gdca_dev_scalars *sc;
};
template <int CAP>
__global__ __launch_bounds__(LOGDET_THREADS) void k_logdet(const BatchArgs<k_logdet_args, CAP> B_)
{
    GDCA_MEMBER(B_);
    const double *__restrict__ piv = a_.piv;
    const int n_real = a_.n_real;
    gdca_dev_scalars *sc = a_.sc;
    __shared__ double part[LOGDET_THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n_real; i += LOGDET_THREADS) acc += log(piv[i]);
    part[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int h = LOGDET_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid == 0) sc->logdet = sc->info == 0 ? part[0] : __longlong_as_double(0x7ff8000000000000ll);
}

void gdca_launch_logdet(hipStream_t s, const double *piv, int n_real, gdca_dev_scalars *sc)
{
    (gdca_launch<k_logdet_args, k_logdet<1>, k_logdet<GDCA_MAXB>>(dim3(1), dim3(LOGDET_THREADS), 0, s, k_logdet_args{piv, n_real, sc}));
}

// L[k] = -(L[k] + c) in place: L holds the energies E, c = 1/2 (n log 2 pi + log det C) comes from the host (one rounding per operation,
// no contraction: the library is built with -ffp-contract=off)
__global__ __launch_bounds__(256) void k_loglik(double *__restrict__ L, int K, double c)
{
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k < K) L[k] = -(L[k] + c);
}

void gdca_launch_loglik(hipStream_t s, double *L, int K, double c)
{
    GDCA_LAUNCH_DIRECT(k_loglik, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, L, K, c);
}
